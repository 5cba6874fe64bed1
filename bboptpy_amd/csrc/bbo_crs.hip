// bbo_crs.hip -- host side of the CRS engine.  Reference behaviour restated on the host:
// CrsSearch::CrsSearch / init / optimize / solution (crs.cpp:40-102).
#include "bbo_crs_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_INIT = 0, K_RANK, K_STEPS, K_EVAL, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:crs_init", "bbo:crs_rank", "bbo:crs_steps", "bbo:crs_eval" };
}

CrsEngine::CrsEngine(const bbo_params &p) :
        WalkEngine(checked(p), "bbo_crs_phase", true)
{
    bbo_crs_params_default(&cp_);
}

// the part of the constructor's arguments that travels in bbo_params
const bbo_params &CrsEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_CRS, "CrsEngine: bad algo");
    BBO_REQUIRE(p.np >= 2 && p.np <= CRS_MAX_NP, "CRS: np must be in [2, 65536]");
    BBO_REQUIRE(p.mfev >= 1, "CRS: mfev must be positive");
    BBO_REQUIRE(p.tol == p.tol, "CRS: tol must not be NaN");
    return p;
}

void CrsEngine::configure(const bbo_crs_params &cp)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_crs_configure after bbo_init");
    BBO_REQUIRE(cp.max_depth >= 1 && cp.max_depth <= (1 << 20), "CRS: max_depth must be in [1, 2^20]");
    BBO_REQUIRE(cp.repair == 0 || cp.repair == 1, "CRS: repair is 0 or 1");
    cp_ = cp;
}

// the threads of crs_steps' workgroup: a lane per coordinate up to 256, as NSHS
int CrsEngine::workgroup() const
{
    return c_.n <= 128 ? 64 : c_.n <= 256 ? 128 : 256;
}

// the steps a population may spend in one fused launch of k iterations
int CrsEngine::launch_evals(int k) const
{
    if (launch_evals_ > 0) return launch_evals_;
    return (int) std::min<long long>((long long) k * CRS_LAUNCH_STEPS_PER_ITERATION, 1 << 30);
}

void CrsEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    (void) guess;   // CRS never reads it (crs.cpp:46-79)
    reject_program(obj, "CRS");
    BBO_REQUIRE(n >= 1 && n <= CRS_MAX_N, "CRS: dimension must be in [1, 512]");
    require_finite_box("CRS draws its pool from [lower, upper] and tests every trial against it: the bounds must be finite",
            n, lower, upper);
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations, np = params_.np;
    BBO_REQUIRE(P <= (1 << 24), "CRS: populations must be <= 2^24");
    CrsConst &c = c_;
    c = CrsConst {};
    c.n = n;
    c.ld = round_up(n, 2);
    c.np = np;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.max_depth = cp_.max_depth;
    c.repair = cp_.repair;
    c.stack_words = (cp_.max_depth + 31) / 32;
    c.tol = params_.tol;
    c.seed = params_.seed;
    mid_generation_ = false;

    const size_t rows = (size_t) P * np;
    X_.alloc(rows * c.ld);
    f_.alloc(rows);
    order_.alloc(rows);
    cand_.alloc((size_t) P * c.ld);
    cand2_.alloc((size_t) P * c.ld);
    value_.alloc(P);
    stack_.alloc((size_t) P * c.stack_words);
    more_.alloc(1);
    tables_.clear();
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    {
        std::vector<double> z((size_t) P * c.ld, 0.);
        cand_.upload(z.data(), z.size());
        cand2_.upload(z.data(), z.size());
        value_.upload(z.data(), P);
        std::vector<uint32_t> zs((size_t) P * c.stack_words, 0u);
        stack_.upload(zs.data(), zs.size());
        std::vector<CrsScal> sc(P);
        std::memset(sc.data(), 0, sizeof(CrsScal) * P);
        for (auto &s : sc) s.fev = np;      // the pool is evaluated (:66-69)
        scal_.upload(sc.data(), P);
    }

    CrsDev &d = d_;
    d = CrsDev {};
    d.X = X_.p; d.f = f_.p; d.order = order_.p; d.cand = cand_.p; d.cand2 = cand2_.p; d.value = value_.p;
    d.stack = stack_.p; d.more = more_.p;
    d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.scal = scal_.p;
    inited_ = true;

    if (obj_.needs_host()) {
        launch_init(0, P, CRS_INIT_DRAW);
        host_evaluate_range(X_, f_, 0, P, np, 0, np, n, c.ld);      // (in row order: :61-70)
    } else {
        launch_init(0, P, CRS_INIT_DRAW | CRS_INIT_EVAL);
    }
    launch_rank(0, P);
    BBO_HIP(hipStreamSynchronize(stream_));
}

void CrsEngine::launch_init(int p0, int pcount, int mode)
{
    timed(K_INIT, [&] {
        hipLaunchKernelGGL(crs_init, dim3(pcount, (c_.np + CRS_INIT_ROWS - 1) / CRS_INIT_ROWS), dim3(256), 0, stream_,
                d_, c_, p0, mode);
    });
}

void CrsEngine::launch_rank(int p0, int pcount)
{
    timed(K_RANK, [&] {
        hipLaunchKernelGGL(crs_rank, dim3(pcount, (c_.np + CRS_RANK_CANDS - 1) / CRS_RANK_CANDS), dim3(256), 0, stream_,
                d_, c_, p0);
    });
}

void CrsEngine::launch_body(int mode, int k, bool begin)
{
    const int b = begin ? 1 : 0;
    const size_t bytes = (size_t) 4 * c_.ld * sizeof(double) + (size_t) round_up(c_.n, 4) * sizeof(int);
    c_.launch_evals = launch_evals(k);
    timed(K_STEPS, [&] {
        switch (workgroup()) {
        case 64: hipLaunchKernelGGL((crs_steps<64>), dim3(c_.npop), dim3(64), bytes, stream_, d_, c_, mode, k, b); break;
        case 128: hipLaunchKernelGGL((crs_steps<128>), dim3(c_.npop), dim3(128), bytes, stream_, d_, c_, mode, k, b); break;
        default: hipLaunchKernelGGL((crs_steps<256>), dim3(c_.npop), dim3(256), bytes, stream_, d_, c_, mode, k, b); break;
        }
    });
}

void CrsEngine::launch_eval_device()
{
    timed(K_EVAL, [&] { hipLaunchKernelGGL(crs_eval, dim3(c_.npop), dim3(64), 0, stream_, d_, c_); });
}

// k iterations of every population with a device objective: launches of bounded length until no
// population is short of its goal (one flag per launch)
void CrsEngine::fused(int k)
{
    for (bool begin = true;; begin = false) {
        BBO_HIP(hipMemsetAsync(more_.p, 0, sizeof(int), stream_));
        launch_body(CRS_FUSED, k, begin);
        BBO_HIP(hipStreamSynchronize(stream_));
        int more = 0;
        more_.download(&more, 1);
        if (!more) break;
    }
}

// one iteration of every population (CRS_FUSED), or the same body from evaluation to evaluation
void CrsEngine::launch_walk(int mode, bool begin)
{
    if (mode == CRS_FUSED) fused(1);
    else launch_body(mode, 1, begin);
}

// bbo_run: `gens` whole iterations per population
void CrsEngine::launch_chunk(int gens)
{
    if (obj_.needs_host()) {
        Engine::launch_chunk(gens);
        return;
    }
    c_.honor_stop = 1;
    fused(gens);
    mid_generation_ = false;
}

// bbo_run cannot wait for a table: an exhausted one ends it
void CrsEngine::inspect(const std::vector<CrsScal> &sc)
{
    for (const auto &s : sc)
        if (s.starved) throw Error(BBO_ERR_STATE, "bbo_run: the injected draws are exhausted (bbo_crs_inject_draws)");
}

void CrsEngine::inject_draws(const double *table, int count)
{
    enter("bbo_crs_inject_draws");
    BBO_HIP(hipStreamSynchronize(stream_));
    const int P = c_.npop, n = c_.n;
    std::vector<CrsScal> sc(P);
    scal_.download(sc.data(), P);
    for (auto &s : sc) {
        s.irec = 0;
        s.starved = 0;
    }
    if (!table) {
        d_.inject = nullptr;
        c_.inject_n = 0;
        // (a record in use stays in use: the draws of a mutation that follows come from the generator)
        scal_.upload(sc.data(), P);
        return;
    }
    const size_t per = (size_t) P * 2 * n;
    BBO_REQUIRE(count > 0 && (size_t) count % per == 0, "bbo_crs_inject_draws: populations * records * 2 n values");
    const size_t nrec = (size_t) count / per;
    for (size_t r = 0; r < (size_t) P * nrec; r++) {
        const double *rec = table + r * 2 * n;
        for (int j = 0; j < n; j++) {
            BBO_REQUIRE(rec[j] == std::floor(rec[j]) && rec[j] >= -1. && rec[j] < c_.np,
                    "bbo_crs_inject_draws: indices are integers in [0, np), -1 where none is drawn");
            BBO_REQUIRE(rec[n + j] >= 0. && rec[n + j] < 1., "bbo_crs_inject_draws: uniforms lie in [0, 1)");
        }
    }
    // a record whose uniforms are not spent belongs to the table before: the walk goes on with a new one
    for (auto &s : sc) s.wused = 1;
    tables_.inject.alloc(0);        // (the table before may have had another length)
    d_.inject = tables_.load(table, (size_t) count);
    c_.inject_n = (int) nrec;
    scal_.upload(sc.data(), P);
}

// the walk of population p starts over: after a set of the pool
void CrsEngine::reset_walk(int p)
{
    CrsScal s;
    scal_.download(&s, 1, p);
    s.stage = CRS_IDLE;
    s.depth = 0;
    s.pending = 0;
    s.starved = 0;
    s.conv = std::fabs(s.fbest - s.fworst) < c_.tol ? 1 : 0;
    scal_.upload(&s, 1, p);
    if (c_.npop == 1) mid_generation_ = false;
}

void CrsEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    CrsScal s;
    scal_.download(&s, 1, population);
    s.conv = std::fabs(s.fbest - s.fworst) < c_.tol ? 1 : 0;    // stop() of the pool (:86-88)
    int best = 0;
    order_.download(&best, 1, (size_t) population * c_.np);
    report_solution(s, X_, ((size_t) population * c_.np + best) * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

int CrsEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const CrsConst &c = c_;
    CrsScal s;
    scal_.download(&s, 1, p);
    const size_t pr = (size_t) p * c.np;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    if (k == "x") return o.rows_by_slot(X_, order_, pr, c.np, c.np, c.n, c.ld);     // rank order
    if (k == "f") return o.vec_by_slot(f_, order_, pr, c.np, c.np);
    if (k == "rows") return o.rows(X_, pr, c.np, c.n, c.ld);                        // in place
    if (k == "order") return o.ints(order_, pr, c.np);
    if (k == "cand") return o.vec(cand_, (size_t) p * c.ld, c.n);
    if (k == "cand2") return o.vec(cand2_, (size_t) p * c.ld, c.n);
    if (k == "value") return o.vec(value_, p, 1);
    if (k == "draws") {
        require_record(c.record > 0, k);
        const int kept = std::min(s.nrec, c.record);
        return o.vec(tables_.draws, (size_t) p * c.record * 2 * c.n, kept * 2 * c.n);
    }
    if (k == "fcand") return o.one(s.ft);
    if (k == "fcand2") return o.one(s.ft2);
    if (k == "fbest") return o.one(s.fbest);
    if (k == "fworst") return o.one(s.fworst);
    if (k == "fev") return o.one(s.fev);
    if (k == "it") return o.one(s.it);
    if (k == "trials") return o.one(s.trials);
    if (k == "muts") return o.one(s.muts);
    if (k == "depth") return o.one(s.depth);
    if (k == "maxdepth") return o.one(s.maxdepth);
    if (k == "stage") return o.one(s.stage);
    if (k == "pending") return o.one(s.pending);
    if (k == "stale") return o.one(s.stale);
    if (k == "flag" || k == "stop") return o.one(s.stop);
    if (k == "conv") return o.one(std::fabs(s.fbest - s.fworst) < c.tol ? 1. : 0.);
    if (k == "nrec") return o.one(s.nrec);
    if (k == "irec") return o.one(s.irec);
    if (k == "starved") return o.one(s.starved);
    if (k == "record_draws") return o.one(c.record);
    if (k == "max_depth") return o.one(c.max_depth);
    if (k == "repair") return o.one(c.repair);
    if (k == "launch_evals") return o.one(launch_evals_);
    if (k == "wg") return o.one(workgroup());
    if (k == "chunk") return o.one(params_.poll_every > 0 ? params_.poll_every : default_poll());
    if (k == "np") return o.one(c.np);
    if (k == "n") return o.one(c.n);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int CrsEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    const CrsConst &c = c_;
    const size_t pr = (size_t) p * c.np;
    auto whole = [&](double lo, double hi) {
        return count == 1 && in[0] == std::floor(in[0]) && in[0] >= lo && in[0] <= hi;
    };
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "record_draws") {      // (the whole handle: every population) 1: CRS_DEFAULT_RECORD records, else so many
        BBO_REQUIRE(whole(0., 4096.), "record_draws: 0, 1 (64 records per iteration) or the records to keep, up to 4096");
        const int want = in[0] == 1. ? CRS_DEFAULT_RECORD : (int) in[0];
        if (want != c.record) tables_.draws.alloc(0);       // (a table of another length)
        c_.record = want;
        d_.draws = tables_.record(want > 0, (size_t) c.npop * want * 2 * c.n);
        return 1;
    }
    if (k == "launch_evals") {
        BBO_REQUIRE(whole(0., 1073741824.), "launch_evals: 0 (8 steps per iteration of the chunk) or the steps of a launch");
        launch_evals_ = (int) in[0];
        return 1;
    }
    if (k == "max_depth") {         // (within the stack bbo_crs_params allocated)
        BBO_REQUIRE(whole(1., (double) c.stack_words * 32), "max_depth: from 1 to the depth the handle was configured with, rounded up to 32");
        c_.max_depth = (int) in[0];
        return 1;
    }
    if (k == "x") {             // rows in place; f, the ranking, the best and the worst follow; fev does not move
        BBO_REQUIRE(count == c.np * c.n, "x: np * n values");
        upload_rows(X_, pr, c.np, c.n, c.ld, in);
        if (obj_.needs_host()) host_evaluate_range(X_, f_, p, 1, c.np, 0, c.np, c.n, c.ld);
        else launch_init(p, 1, CRS_INIT_EVAL);
        launch_rank(p, 1);
        BBO_HIP(hipStreamSynchronize(stream_));
        reset_walk(p);
        return count;
    }
    if (k == "f") {             // values of the rows in place; the ranking follows; nothing is evaluated
        BBO_REQUIRE(count == c.np, "f: np values");
        std::vector<double> fh(in, in + count);
        nan_to_inf(fh.data(), count);
        f_.upload(fh.data(), c.np, pr);
        launch_rank(p, 1);
        BBO_HIP(hipStreamSynchronize(stream_));
        reset_walk(p);
        return count;
    }
    if (k == "value") {         // (what bbo_crs_phase 2 absorbs)
        BBO_REQUIRE(count == 1, "value: one value");
        double v = in[0];
        nan_to_inf(&v, 1);
        value_.upload(&v, 1, p);
        return 1;
    }
    if (k == "fev" || k == "stale") {       // (the budget test looks at fev after the next iteration)
        BBO_REQUIRE(whole(0., 2147483646.), "fev, stale: one non-negative integer");
        CrsScal s;
        scal_.download(&s, 1, p);
        (k == "fev" ? s.fev : s.stale) = (int) in[0];
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_crs_engine(const bbo_params &p)
{
    return new CrsEngine(p);
}

} // namespace bbo
