// bbo_pikaia.hip -- host side of the PIKAIA engine.  Reference behaviour restated on the host:
// PikaiaSearch::PikaiaSearch / init / iterate / optimize / solution (pikaia.cpp:18-148).
#include "bbo_pikaia_kernels.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_INIT = 0, K_BREED, K_NEWPOP, K_COPY, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:pikaia_init", "bbo:pikaia_breed", "bbo:pikaia_newpop",
        "bbo:pikaia_copy" };
}

PikaiaEngine::PikaiaEngine(const bbo_params &p) :
        Engine(checked(p))
{
    bbo_pikaia_params_default(&gp_);
}

// the part of the constructor's arguments that travels in bbo_params: np, ngen (mfev), nd (h)
const bbo_params &PikaiaEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_PIKAIA, "PikaiaEngine: bad algo");
    BBO_REQUIRE(p.np >= 2 && p.np <= PIKAIA_MAX_NP, "PIKAIA: np must be in [2, 4096]");
    BBO_REQUIRE(p.np % 2 == 0, "PIKAIA: np must be even (the reference leaves the last row of an odd new "
            "population unwritten: a zero vector)");
    BBO_REQUIRE(p.h >= 1 && p.h <= PIKAIA_MAX_ND, "PIKAIA: nd must be in [1, 9] (int(ph 10^nd) overflows an int "
            "from nd = 10)");
    BBO_REQUIRE(p.mfev >= 1, "PIKAIA: ngen must be >= 1");
    BBO_REQUIRE((long long) p.np + (long long) p.mfev * (p.np + 1) <= (long long) INT_MAX,
            "PIKAIA: np + ngen (np + 1) evaluations must fit the int counter");
    return p;
}

void PikaiaEngine::configure(const bbo_pikaia_params &gp)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_pikaia_configure after bbo_init");
    BBO_REQUIRE(gp.irep == 1, "PIKAIA: irep must be 1 (full generational replacement).  The steady-state plans "
            "irep = 2, 3 insert every child at once and the next select reads the ranks that insertion left: a "
            "sequential walk with the evaluations inside it, which is not built");
    BBO_REQUIRE(gp.imut >= 1 && gp.imut <= 6, "PIKAIA: imut must be in [1, 6]");
    BBO_REQUIRE(gp.ielite == 0 || gp.ielite == 1, "PIKAIA: ielite is 0 or 1");
    BBO_REQUIRE(gp.pcross >= 0. && gp.pcross <= 1., "PIKAIA: pcross must lie in [0, 1]");
    BBO_REQUIRE(gp.pmut >= 0. && gp.pmut <= 1., "PIKAIA: pmut must lie in [0, 1]");
    BBO_REQUIRE(gp.pmutmn >= 0. && gp.pmutmn <= 1., "PIKAIA: pmutmn must lie in [0, 1]");
    BBO_REQUIRE(gp.pmutmx >= 0. && gp.pmutmx <= 1., "PIKAIA: pmutmx must lie in [0, 1]");
    BBO_REQUIRE(gp.pmutmn <= gp.pmutmx, "PIKAIA: pmutmn must not exceed pmutmx");
    BBO_REQUIRE(gp.fdif >= 0. && gp.fdif <= 1., "PIKAIA: fdif must lie in [0, 1] (beyond 1 the weights of "
            "select turn negative)");
    BBO_REQUIRE(gp.repair == 0 || gp.repair == 1, "PIKAIA: repair is 0 or 1");
    BBO_REQUIRE(gp.raw == 0 || gp.raw == 1, "PIKAIA: raw is 0 or 1");
    BBO_REQUIRE(gp.substream >= 0 && gp.substream < (1 << 24), "PIKAIA: substream must be in [0, 2^24)");
    gp_ = gp;
}

void PikaiaEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    (void) guess;   // the reference never reads it (pikaia.cpp:34-69)
    BBO_REQUIRE(n >= 1 && n <= PIKAIA_MAX_N, "PIKAIA: dimension must be in [1, 512]");
    if (!gp_.raw)
        require_finite_box("PIKAIA maps its phenotypes from the unit cube onto [lower, upper]: the bounds must be "
                "finite (raw=True hands the objective the unit cube itself)", n, lower, upper);
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations, np = params_.np;
    BBO_REQUIRE(P <= 65535, "PIKAIA: populations must be <= 65535 (a grid dimension)");
    PikaiaConst &c = c_;
    c = PikaiaConst {};
    c.n = n;
    c.ld = round_up(n, 2);
    c.np = np;
    c.nd = params_.h;
    c.ngen = params_.mfev;
    c.imut = gp_.imut;
    c.ielite = gp_.ielite;
    c.repair = gp_.repair;
    c.raw = gp_.raw;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.prog = obj.is_program() ? 1 : 0;
    c.npop = P;
    c.sub0 = gp_.substream;
    const PikaiaTable t = pikaia_table(n, np, c.nd);
    c.table = (int) t.len;
    // 10^nd and 10^-nd as the reference's encode and decode form them (:273, :286)
    c.z = std::pow(10., c.nd);
    c.zinv = std::pow(10., -c.nd);
    c.zi = (int) c.z;
    c.pcross = gp_.pcross; c.pmutmn = gp_.pmutmn; c.pmutmx = gp_.pmutmx; c.fdif = gp_.fdif;
    c.seed = params_.seed;

    const size_t rows = (size_t) P * np;
    ph_.alloc(rows * c.ld); x_.alloc(rows * c.ld); newph_.alloc(rows * c.ld); newx_.alloc(rows * c.ld);
    fitns_.alloc(rows); newf_.alloc(rows); cum_.alloc(rows); best_.alloc((size_t) P * c.ld);
    order_.alloc(rows); rank_.alloc(rows); parents_.alloc(rows); cross_.alloc(rows); mode_.alloc(rows);
    tables_.clear();
    record_ = false;
    scal_.alloc(P);
    // raw never reads the box: the kernels get the unit cube in its place
    std::vector<double> lo(n, 0.), hi(n, 1.);
    upload_box(n, c.ld, gp_.raw ? lo.data() : lower, gp_.raw ? hi.data() : upper, obj);
    {
        std::vector<PikaiaScal> sc(P);
        std::memset(sc.data(), 0, sizeof(PikaiaScal) * P);
        for (auto &s : sc) {
            s.pmut = gp_.pmut;
            s.fbest = -std::numeric_limits<double>::infinity();
        }
        scal_.upload(sc.data(), P);
        std::vector<int> z(rows, -1);
        parents_.upload(z.data(), rows);
        cross_.upload(z.data(), rows);
        mode_.upload(z.data(), rows);
    }

    PikaiaDev &d = d_;
    d = PikaiaDev {};
    d.ph = ph_.p; d.x = x_.p; d.fitns = fitns_.p; d.newph = newph_.p; d.newx = newx_.p; d.newf = newf_.p;
    d.cum = cum_.p; d.best = best_.p; d.order = order_.p; d.rank = rank_.p; d.parents = parents_.p;
    d.cross = cross_.p; d.mode = mode_.p;
    d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.scal = scal_.p;

    if (obj_.is_program()) {
        prog_.bind(obj_.program, params_.device, n, P);
        std::vector<ProgPlan> plan(P);
        for (int p = 0; p < P; p++)
            plan[p] = ProgPlan { newx_.p + (size_t) p * np * c.ld, newf_.p + (size_t) p * np, np, c.ld };
        prog_.upload_plan(plan);
        // a second table of one row per population, so that the elite test costs one evaluation
        prog_row0_.bind(obj_.program, params_.device, n, P);
        for (auto &e : plan) e.rows = 1;
        prog_row0_.upload_plan(plan);
    } else {
        prog_.unbind();
        prog_row0_.unbind();
    }
    inited_ = true;
    c.honor_stop = 0;

    timed(K_INIT, [&] { hipLaunchKernelGGL(pikaia_init, dim3(np, P), dim3(64), 0, stream_, d_, c_); });
    evaluate_new(false, np);
    launch_newpop(PIKAIA_INIT);
    launch_copy();
    BBO_HIP(hipStreamSynchronize(stream_));
}

// The values of the first `rows` new rows where the breeding kernel has not formed them: an objective
// program in one launch (all np rows, or row 0 alone through its own plan), a host objective row by row in
// row order.  A callable's NaN stays a NaN; a program's arrives as +inf (pikaia_fitness ranks both worst).
void PikaiaEngine::evaluate_new(bool honor_stop, int rows)
{
    if (obj_.fused()) return;
    if (obj_.is_program()) {
        (rows == 1 ? prog_row0_ : prog_).launch(stream_, rows, honor_stop ? (const void*) &d_.scal[0].stop : nullptr, (int) sizeof(PikaiaScal),
                &prog_timer_);
        return;
    }
    BBO_HIP(hipStreamSynchronize(stream_));
    const int P = c_.npop, np = c_.np, ld = c_.ld;
    std::vector<PikaiaScal> sc(P);
    scal_.download(sc.data(), P);
    std::vector<double> xh((size_t) rows * ld), fh(rows);
    for (int p = 0; p < P; p++) {
        if (honor_stop && sc[p].stop) continue;
        newx_.download(xh.data(), xh.size(), (size_t) p * np * ld);
        for (int r = 0; r < rows; r++) obj_.eval_host(xh.data() + (size_t) r * ld, 1, c_.n, ld, &fh[r]);
        newf_.upload(fh.data(), rows, (size_t) p * np);
    }
}

void PikaiaEngine::launch_newpop(int mode)
{
    const int m = rank_sort_m(c_.np);
    const size_t lds = (size_t) 12 * std::max(m, 1024);
    timed(K_NEWPOP, [&] {
        hipLaunchKernelGGL(pikaia_newpop, dim3(c_.npop), dim3(sort_threads(m)), lds, stream_, d_, c_, mode, m);
    });
}

void PikaiaEngine::launch_copy()
{
    timed(K_COPY, [&] { hipLaunchKernelGGL(pikaia_copy, dim3(c_.np, c_.npop), dim3(64), 0, stream_, d_, c_); });
}

// one iterate() of the reference in every population (:71-123)
void PikaiaEngine::generation(bool honor_stop)
{
    c_.honor_stop = honor_stop ? 1 : 0;
    const int np = c_.np, P = c_.npop;
    timed(K_BREED, [&] { hipLaunchKernelGGL(pikaia_breed, dim3(np / 2, P), dim3(64), 0, stream_, d_, c_); });
    if (obj_.fused()) {
        launch_newpop(PIKAIA_ELITE | PIKAIA_REST);
    } else if (c_.ielite && !c_.repair) {
        // the reference's order (:574-587): new row 1 for the elite test, then rows 1 .. np as they stand
        evaluate_new(honor_stop, 1);
        launch_newpop(PIKAIA_ELITE);
        evaluate_new(honor_stop, np);
        launch_newpop(PIKAIA_REST);
    } else {
        evaluate_new(honor_stop, np);
        launch_newpop(PIKAIA_ELITE | PIKAIA_REST);
    }
    launch_copy();
}

void PikaiaEngine::inject_draws(const double *table, int count)
{
    enter("bbo_pikaia_inject_draws");
    BBO_HIP(hipStreamSynchronize(stream_));
    if (!table) {
        d_.inject = nullptr;
        return;
    }
    const int P = c_.npop;
    BBO_REQUIRE(count > 0 && (size_t) count == (size_t) P * c_.table,
            "bbo_pikaia_inject_draws: populations * (np / 2) * (69 + 2 (1 + 2 n nd)) values");
    for (size_t q = 0; q < (size_t) count; q++)
        BBO_REQUIRE(table[q] == -1. || (table[q] >= 0. && table[q] < 1.),
                "bbo_pikaia_inject_draws: uniforms lie in [0, 1), -1 where none is drawn");
    const PikaiaTable t = pikaia_table(c_.n, c_.np, c_.nd);
    // every slot the generation will read holds a draw (checked against pmut as it stands: a table is for
    // the generation that follows)
    std::vector<PikaiaScal> sc(P);
    scal_.download(sc.data(), P);
    for (int p = 0; p < P; p++)
        for (int mt = 0; mt < c_.np / 2; mt++) {
            const double *tm = table + (size_t) p * c_.table + (size_t) mt * t.per_mating;
            BBO_REQUIRE(tm[0] >= 0. && tm[t.p2] >= 0. && tm[t.x] >= 0.,
                    "bbo_pikaia_inject_draws: every mating draws its first parent, a second and the crossover coin");
            if (tm[t.x] < c_.pcross)
                BBO_REQUIRE(tm[t.x + 1] >= 0. && tm[t.x + 2] >= 0. && (tm[t.x + 2] < 0.5 || tm[t.x + 3] >= 0.),
                        "bbo_pikaia_inject_draws: a mating that crosses draws ispl, the coin and, for two points, ispl2");
            for (int ch = 0; ch < 2; ch++) {
                const double *tc = tm + t.child + (size_t) ch * t.per_child;
                BBO_REQUIRE(c_.imut < 4 || tc[0] >= 0., "bbo_pikaia_inject_draws: imut >= 4 draws the coin of every child");
                for (int q = 0; q < t.loci; q++)
                    BBO_REQUIRE(tc[1 + q] >= 0. && (!(tc[1 + q] < sc[p].pmut) || tc[1 + t.loci + q] >= 0.),
                            "bbo_pikaia_inject_draws: every locus draws its uniform, and its value where that is below pmut");
            }
        }
    d_.inject = tables_.load(table, (size_t) P * c_.table);
}

void PikaiaEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    PikaiaScal s;
    scal_.download(&s, 1, population);
    s.conv = 1;     // :131: converged = true, always
    int ib = 0;
    order_.download(&ib, 1, (size_t) population * c_.np + c_.np - 1);
    // :129: the best row of the population as it stands
    report_solution(s, x_, ((size_t) population * c_.np + ib) * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

int PikaiaEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const PikaiaConst &c = c_;
    PikaiaScal s;
    scal_.download(&s, 1, p);
    const size_t pr = (size_t) p * c.np;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    {
        const int r = prog_get(k, out, cap);
        if (r >= 0) return r;
    }
    if (k == "ph") return o.rows(ph_, pr, c.np, c.n, c.ld);
    if (k == "x") return o.rows(x_, pr, c.np, c.n, c.ld);
    if (k == "fitns") return o.vec(fitns_, pr, c.np);
    if (k == "order") return o.ints(order_, pr, c.np);
    if (k == "rank") return o.ints(rank_, pr, c.np);
    if (k == "cum") return o.vec(cum_, pr, c.np);
    if (k == "new_ph") return o.rows(newph_, pr, c.np, c.n, c.ld);
    if (k == "new_x") return o.rows(newx_, pr, c.np, c.n, c.ld);
    if (k == "new_f") return o.vec(newf_, pr, c.np);
    if (k == "parents") return o.ints(parents_, pr, c.np);
    if (k == "cross") return o.ints(cross_, pr, c.np);
    if (k == "mode") return o.ints(mode_, pr, c.np);
    if (k == "xbest") return o.vec(best_, (size_t) p * c.ld, c.n);
    if (k == "draws") {
        require_record(record_, k);
        return o.vec(tables_.draws, (size_t) p * c.table, c.table);
    }
    if (k == "fbest") return o.one(c.raw ? s.fbest : -s.fbest);     // the objective's scale
    if (k == "pmut") return o.one(s.pmut);
    if (k == "rdif") return o.one(s.rdif);
    if (k == "ig") return o.one(s.ig);
    if (k == "fev") return o.one(s.fev);
    if (k == "elite") return o.one(s.elite);
    if (k == "flag" || k == "stop") return o.one(s.stop);
    if (k == "conv") return o.one(1.);
    if (k == "record_draws") return o.one(record_ ? 1. : 0.);
    if (k == "table_len") return o.one(c.table);
    if (k == "repair") return o.one(c.repair);
    if (k == "raw") return o.one(c.raw);
    if (k == "substream") return o.one(c.sub0);
    if (k == "ngen") return o.one(c.ngen);
    if (k == "nd") return o.one(c.nd);
    if (k == "z") return o.one(c.z);
    if (k == "zinv") return o.one(c.zinv);
    if (k == "np") return o.one(c.np);
    if (k == "n") return o.one(c.n);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int PikaiaEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    const PikaiaConst &c = c_;
    const size_t pr = (size_t) p * c.np;
    auto whole = [&](double lo, double hi) {
        return count == 1 && in[0] == std::floor(in[0]) && in[0] >= lo && in[0] <= hi;
    };
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    {
        const int r = prog_set(k, in, count);
        if (r >= 0) return r;
    }
    if (k == "record_draws") {      // (the whole handle) the draws of the last generation in the layout of inject_draws
        BBO_REQUIRE(whole(0., 1.), "record_draws: 0 or 1");
        record_ = in[0] != 0.;
        d_.draws = tables_.record(record_, (size_t) c.npop * c.table);
        return 1;
    }
    // a whole state, key by key: nothing is evaluated and nothing follows from what is written
    if (k == "ph") {        // the phenotypes and the points they map to
        BBO_REQUIRE(count == c.np * c.n, "ph: np * n values");
        std::vector<double> xm(count);
        for (int q = 0; q < count; q++) {
            BBO_REQUIRE(in[q] >= 0. && in[q] <= 1., "ph: phenotypes lie in [0, 1]");
            const int i = q % c.n;
            // (the kernels' map, bbo_pikaia_kernels.hpp: one multiply, one add)
            volatile double w = upper_h_[i] - lower_h_[i];
            volatile double sft = in[q] * w;
            xm[q] = c.raw ? in[q] : lower_h_[i] + sft;
        }
        upload_rows(ph_, pr, c.np, c.n, c.ld, in);
        upload_rows(x_, pr, c.np, c.n, c.ld, xm.data());
        return count;
    }
    if (k == "fitns") {
        BBO_REQUIRE(count == c.np, "fitns: np values");
        for (int q = 0; q < count; q++) BBO_REQUIRE(in[q] == in[q], "fitns: not NaN");
        fitns_.upload(in, c.np, pr);
        return count;
    }
    if (k == "order") {     // rank -> row; the ranks and select's running sums follow from it
        BBO_REQUIRE(count == c.np, "order: np values");
        const std::vector<int> ord = permutation_of(in, c.np, "order: a permutation of 0 .. np - 1");
        std::vector<int> rk(c.np);
        for (int r = 0; r < c.np; r++) rk[ord[r]] = r;
        std::vector<double> cum(c.np);
        volatile double rt = 0.;
        for (int r = 0; r < c.np; r++) {
            volatile double w = c.fdif * (c.np + 1 - 2 * (c.np - rk[r]));
            rt = rt + (c.np + 1);
            rt = rt + w;
            cum[r] = rt;
        }
        order_.upload(ord.data(), c.np, pr);
        rank_.upload(rk.data(), c.np, pr);
        cum_.upload(cum.data(), c.np, pr);
        return count;
    }
    if (k == "xbest") {
        BBO_REQUIRE(count == c.n, "xbest: n values");
        std::vector<double> x(c.ld, 0.);
        std::copy(in, in + c.n, x.begin());
        best_.upload(x.data(), c.ld, (size_t) p * c.ld);
        return count;
    }
    PikaiaScal s;
    scal_.download(&s, 1, p);
    if (k == "pmut") {
        BBO_REQUIRE(count == 1 && in[0] >= 0. && in[0] <= 1., "pmut: one value in [0, 1]");
        s.pmut = in[0];
    } else if (k == "fbest") {
        BBO_REQUIRE(count == 1 && in[0] == in[0], "fbest: one value, not NaN");
        s.fbest = c.raw ? in[0] : -in[0];
    } else if (k == "fev") {
        BBO_REQUIRE(whole(0., 2147483646.), "fev: one non-negative integer");
        s.fev = (int) in[0];
    } else if (k == "ig") {     // (the stop test looks at ig after the next generation)
        BBO_REQUIRE(whole(1., 2147483646.), "ig: one positive integer");
        s.ig = (int) in[0];
    } else {
        throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
    }
    scal_.upload(&s, 1, p);
    return 1;
}

Optimizer* make_pikaia_engine(const bbo_params &p)
{
    return new PikaiaEngine(p);
}

} // namespace bbo
