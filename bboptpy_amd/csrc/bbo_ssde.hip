// bbo_ssde.hip -- host side of the SSDE engine.  Reference behaviour restated on the host:
// SSDESearch::SSDESearch / init / optimize / solution (ssde.cpp:46-132, :363-381).
#include "bbo_ssde_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_INIT = 0, K_GENERATION, K_EVAL, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:ssde_init", "bbo:ssde_generation", "bbo:ssde_eval" };
}

SsdeEngine::SsdeEngine(const bbo_params &p) :
        WalkEngine(checked(p), "bbo_ssde_phase", false)
{
    bbo_ssde_params_default(&sp_);
}

// the part of the constructor's arguments that travels in bbo_params; what depends on bbo_ssde_configure
// is checked by init
const bbo_params &SsdeEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_SSDE, "SsdeEngine: bad algo");
    BBO_REQUIRE(p.mfev >= 1, "SSDE: mfev must be positive");
    BBO_REQUIRE(std::isfinite(p.tol), "SSDE: tol must be finite");
    return p;
}

void SsdeEngine::configure(const bbo_ssde_params &sp)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_ssde_configure after bbo_init");
    sp_ = sp;
}

// the threads of ssde_generation's workgroup: a lane per coordinate, one wavefront up to n = 64
int SsdeEngine::workgroup() const
{
    return c_.n <= 64 ? 64 : c_.n <= 128 ? 128 : 256;
}

void SsdeEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    (void) guess;   // SSDE never reads it (ssde.cpp:59-132)
    reject_program(obj, "SSDE");
    BBO_REQUIRE(n >= 1 && n <= SSDE_MAX_N, "SSDE: dimension must be in [1, 512]");
    require_finite_box("SSDE draws its pool from [lower, upper] and clamps to it: the bounds must be finite",
            n, lower, upper);
    const int P = params_.populations, npinit = params_.np;
    // (sample3 draws three members besides i, :459-472)
    BBO_REQUIRE(npinit >= SSDE_MIN_NP && npinit <= SSDE_MAX_NP, "SSDE: npinit must be in [4, 4096]");
    BBO_REQUIRE(sp_.npmin >= SSDE_MIN_NP && sp_.npmin <= npinit, "SSDE: npmin must be in [4, npinit]");
    BBO_REQUIRE(sp_.h >= 1 && sp_.h <= SSDE_MAX_H, "SSDE: h must be in [1, 65536]");
    // (pbest is drawn from [0, int(ptop np)] inclusive, :169-170: ptop = 1 would read past the pool)
    BBO_REQUIRE(sp_.ptop > 0. && sp_.ptop < 1., "SSDE: ptop must lie in (0, 1)");
    BBO_REQUIRE(sp_.patience >= 0, "SSDE: patience must not be negative");
    BBO_REQUIRE((sp_.usede == 0 || sp_.usede == 1) && (sp_.repaircr == 0 || sp_.repaircr == 1),
            "SSDE: usede and repaircr are 0 or 1");
    BBO_REQUIRE(P <= (1 << 24), "SSDE: populations must be <= 2^24");
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int keep_sub = c_.sub0;
    SsdeConst &c = c_;
    c = SsdeConst {};
    c.n = n;
    c.ld = round_up(n, 2);
    c.npinit = npinit;
    c.nrows = sp_.usede ? 2 * npinit : npinit;
    c.H = sp_.h;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.sub0 = keep_sub;
    c.patience = sp_.patience;
    c.npmin = sp_.npmin;
    c.usede = sp_.usede;
    c.repaircr = sp_.repaircr;
    c.ptop = sp_.ptop;
    c.tol = params_.tol;
    c.seed = params_.seed;

    const size_t rows = (size_t) P * c.nrows, mem = (size_t) P * npinit, hist = (size_t) P * c.H;
    x_.alloc(rows * c.ld);
    f_.alloc(rows); order_.alloc(rows); order2_.alloc(rows);
    L1_.alloc(hist); L2_.alloc(hist); LCR_.alloc(hist);
    SR_.alloc(mem); SC_.alloc(mem); w_.alloc(mem); SCR_.alloc(mem); wCR_.alloc(mem); radius_.alloc(mem);
    perm_.alloc((size_t) P * c.ld); cand_.alloc((size_t) P * c.ld);
    fcand_.alloc(P);
    tables_.clear();
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    {
        std::vector<double> zx(rows * c.ld, 0.);
        x_.upload(zx.data(), zx.size());        // (the padding columns)
        std::vector<SsdeScal> sc(P);
        std::memset(sc.data(), 0, sizeof(SsdeScal) * P);
        scal_.upload(sc.data(), P);
    }

    SsdeDev &d = d_;
    d = SsdeDev {};
    d.x = x_.p; d.f = f_.p; d.order = order_.p; d.order2 = order2_.p;
    d.L1 = L1_.p; d.L2 = L2_.p; d.LCR = LCR_.p;
    d.SR = SR_.p; d.SC = SC_.p; d.w = w_.p; d.SCR = SCR_.p; d.wCR = wCR_.p; d.radius = radius_.p;
    d.perm = perm_.p; d.cand = cand_.p; d.fcand = fcand_.p;
    d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.scal = scal_.p;
    inited_ = true;
    mid_generation_ = false;
    seed_pool(0, P);
}

// :87-131 the pool of the populations p0 .. p0 + pcount - 1, drawn from their sub-streams
void SsdeEngine::seed_pool(int p0, int pcount)
{
    const int draw = SSDE_INIT_DRAW | (c_.usede ? SSDE_INIT_OPP : 0), rank = SSDE_INIT_RESET | SSDE_INIT_SORT;
    if (obj_.needs_host()) {
        launch_init(p0, pcount, draw, 0, 0);
        // (the points, then their opposites: :95, :107)
        host_evaluate_range(x_, f_, p0, pcount, c_.nrows, 0, c_.nrows, c_.n, c_.ld);
        launch_init(p0, pcount, rank, 0, c_.nrows);
    } else {
        launch_init(p0, pcount, draw | SSDE_INIT_EVAL | rank, 0, c_.nrows);
    }
    BBO_HIP(hipStreamSynchronize(stream_));
}

void SsdeEngine::launch_init(int p0, int pcount, int mode, int r0, int r1)
{
    timed(K_INIT, [&] { hipLaunchKernelGGL(ssde_init, dim3(pcount), dim3(256), 0, stream_, d_, c_, p0, mode, r0, r1); });
}

// one iterate() of every population (SSDE_FUSED), or the same body from evaluation to evaluation
void SsdeEngine::launch_walk(int mode, bool begin)
{
    const int b = begin ? 1 : 0;
    const size_t bytes = (size_t) 5 * c_.ld * sizeof(double) + (size_t) 2 * c_.ld * sizeof(int);
    timed(K_GENERATION, [&] {
        switch (workgroup()) {
        case 64: hipLaunchKernelGGL((ssde_generation<64>), dim3(c_.npop), dim3(64), bytes, stream_, d_, c_, mode, b); break;
        case 128: hipLaunchKernelGGL((ssde_generation<128>), dim3(c_.npop), dim3(128), bytes, stream_, d_, c_, mode, b); break;
        default: hipLaunchKernelGGL((ssde_generation<256>), dim3(c_.npop), dim3(256), bytes, stream_, d_, c_, mode, b); break;
        }
    });
}

void SsdeEngine::launch_eval_device()
{
    timed(K_EVAL, [&] { hipLaunchKernelGGL(ssde_eval, dim3(c_.npop), dim3(64), 0, stream_, d_, c_); });
}

void SsdeEngine::inject_draws(const double *table, int count)
{
    enter("bbo_ssde_inject_draws");
    BBO_HIP(hipStreamSynchronize(stream_));
    if (!table) {
        d_.inject = nullptr;
        return;
    }
    const int n = c_.n, npinit = c_.npinit;
    const size_t len = table_len(), want = (size_t) c_.npop * len, rec = SSDE_REC_HEAD + 3 * (size_t) n;
    BBO_REQUIRE(count >= 0 && (size_t) count == want,
            "bbo_ssde_inject_draws: populations * (n + npinit * (9 + 3 n)) values");
    auto unit = [](double u) { return u >= 0. && u < 1.; };
    auto index = [](double v, int below) { return v >= 0. && v < below && v == std::floor(v); };
    for (int p = 0; p < c_.npop; p++) {
        const double *t = table + (size_t) p * len;
        permutation_of(t, n, "bbo_ssde_inject_draws: perm is a permutation of 0 .. n - 1");
        for (int i = 0; i < npinit; i++) {
            const double *m = t + n + (size_t) i * rec;
            BBO_REQUIRE(index(m[0], c_.H), "bbo_ssde_inject_draws: iL lies in [0, h)");
            BBO_REQUIRE(index(m[2], npinit) && index(m[3], npinit) && index(m[4], npinit) && index(m[5], npinit),
                    "bbo_ssde_inject_draws: p, q, r and pbest are members");
            BBO_REQUIRE(m[6] >= 0. && m[6] <= 1., "bbo_ssde_inject_draws: ci lies in (0, 1] (0 where none is drawn)");
            BBO_REQUIRE(std::isfinite(m[1]) && std::isfinite(m[7]), "bbo_ssde_inject_draws: normals are finite");
            BBO_REQUIRE(index(m[8], n), "bbo_ssde_inject_draws: j0 is a coordinate");
            for (size_t j = SSDE_REC_HEAD; j < rec; j++)
                BBO_REQUIRE(unit(m[j]), "bbo_ssde_inject_draws: uniforms lie in [0, 1)");
        }
    }
    d_.inject = tables_.load(table, want);
}

void SsdeEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    SsdeScal s;
    scal_.download(&s, 1, population);
    int best = 0;
    order_.download(&best, 1, (size_t) population * c_.nrows);
    report_solution(s, x_, ((size_t) population * c_.nrows + best) * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

int SsdeEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const SsdeConst &c = c_;
    SsdeScal s;
    scal_.download(&s, 1, p);
    const size_t pr = (size_t) p * c.nrows;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    if (k == "x") return o.rows_by_slot(x_, order_, pr, s.np, c.nrows, c.n, c.ld);
    if (k == "f") return o.vec_by_slot(f_, order_, pr, s.np, c.nrows);
    if (k == "order") return o.ints(order_, pr, s.np);
    if (k == "L1") return o.vec(L1_, (size_t) p * c.H, c.H);
    if (k == "L2") return o.vec(L2_, (size_t) p * c.H, c.H);
    if (k == "LCR") return o.vec(LCR_, (size_t) p * c.H, c.H);
    if (k == "perm") return o.ints(perm_, (size_t) p * c.ld, c.n);
    if (k == "cand") return o.vec(cand_, (size_t) p * c.ld, c.n);
    if (k == "fcand") return o.vec(fcand_, p, 1);
    if (k == "draws") {
        require_record(c.record, k);
        return o.vec(tables_.draws, (size_t) p * table_len(), (int) table_len());
    }
    if (k == "k") return o.one(s.k);
    if (k == "kCR") return o.one(s.kCR);
    if (k == "np") return o.one(s.np);
    if (k == "fev") return o.one(s.fev);
    if (k == "gen") return o.one(s.gen);
    if (k == "convcount") return o.one(s.convcount);
    if (k == "flag" || k == "stop") return o.one(s.stop);
    if (k == "conv") return o.one(s.conv);
    if (k == "pending") return o.one(s.pending);
    if (k == "stage") return o.one(s.stage);
    if (k == "member") return o.one(s.mi);
    if (k == "record_draws") return o.one(c.record);
    if (k == "substream") return o.one(c.sub0);
    if (k == "wg") return o.one(workgroup());
    if (k == "npinit") return o.one(c.npinit);
    if (k == "n") return o.one(c.n);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

// set() of one of the three memories
void SsdeEngine::set_memory(DevBuf<double> &b, int p, const double *in, int count, const char *what)
{
    BBO_REQUIRE(count == c_.H, std::string(what) + ": h values");
    for (int i = 0; i < count; i++) BBO_REQUIRE(std::isfinite(in[i]), std::string(what) + ": finite values");
    b.upload(in, count, (size_t) p * c_.H);
}

int SsdeEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    const SsdeConst &c = c_;
    auto whole = [&](int below) {
        return count == 1 && in[0] >= 0. && in[0] == std::floor(in[0]) && in[0] < below;
    };
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "record_draws") {      // (the whole handle: every population)
        BBO_REQUIRE(count == 1, "record_draws: one value");
        c_.record = in[0] != 0. ? 1 : 0;
        d_.draws = tables_.record(c_.record, (size_t) c.npop * table_len());
        return 1;
    }
    if (k == "substream") {     // the sub-stream of population 0; the pool is drawn again from it
        BBO_REQUIRE(count == 1 && in[0] >= 0. && in[0] == std::floor(in[0]) && in[0] + c.npop <= (1 << 24),
                "substream: one integer in [0, 2^24 - populations]");
        c_.sub0 = (int) in[0];
        mid_generation_ = false;
        seed_pool(0, c.npop);
        return 1;
    }
    if (k == "x") {             // m rows in place, ranked from their values: np = m
        BBO_REQUIRE(count % c.n == 0 && count / c.n >= SSDE_MIN_NP && count / c.n <= c.npinit,
                "x: m * n values, 4 <= m <= npinit");
        const int m = count / c.n;
        upload_rows(x_, (size_t) p * c.nrows, m, c.n, c.ld, in);
        if (c.npop == 1) mid_generation_ = false;   // (the generation in progress, if any, is abandoned)
        if (obj_.needs_host()) {
            host_evaluate_range(x_, f_, p, 1, c.nrows, 0, m, c.n, c.ld);
            launch_init(p, 1, SSDE_INIT_SORT, 0, m);
        } else {
            launch_init(p, 1, SSDE_INIT_EVAL | SSDE_INIT_SORT, 0, m);
        }
        BBO_HIP(hipStreamSynchronize(stream_));
        return count;
    }
    if (k == "L1") return set_memory(L1_, p, in, count, "L1"), count;
    if (k == "L2") {
        for (int i = 0; i < count; i++) BBO_REQUIRE(in[i] > 0., "L2: positive values");
        return set_memory(L2_, p, in, count, "L2"), count;
    }
    if (k == "LCR") return set_memory(LCR_, p, in, count, "LCR"), count;
    if (k == "perm") {          // the next generation keeps it
        BBO_REQUIRE(count == c.n, "perm: n values");
        perm_.upload(permutation_of(in, c.n, "perm: a permutation of 0 .. n - 1").data(), c.n, (size_t) p * c.ld);
        SsdeScal s;
        scal_.download(&s, 1, p);
        s.keep_perm = 1;
        scal_.upload(&s, 1, p);
        return count;
    }
    if (k == "cand") {          // (what bbo_ssde_phase 1 evaluates)
        BBO_REQUIRE(count == c.n, "cand: n values");
        cand_.upload(in, c.n, (size_t) p * c.ld);
        return count;
    }
    if (k == "fcand") {         // (what bbo_ssde_phase 2 absorbs)
        BBO_REQUIRE(count == 1, "fcand: one value");
        double v = in[0];
        nan_to_inf(&v, 1);
        fcand_.upload(&v, 1, p);
        return 1;
    }
    if (k == "k" || k == "kCR" || k == "fev" || k == "convcount") {
        SsdeScal s;
        scal_.download(&s, 1, p);
        if (k == "fev") {       // (R reads it at every member; the budget test after the next generation)
            BBO_REQUIRE(whole(2147483647), "fev: one non-negative integer");
            s.fev = (int) in[0];
        } else if (k == "convcount") {
            BBO_REQUIRE(whole(2147483647), "convcount: one non-negative integer");
            s.convcount = (int) in[0];
        } else {
            BBO_REQUIRE(whole(c.H + 1) && in[0] >= 1., k + ": one integer in [1, h]");
            (k == "k" ? s.k : s.kCR) = (int) in[0];
        }
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_ssde_engine(const bbo_params &p)
{
    return new SsdeEngine(p);
}

} // namespace bbo
