// bbo_de.hip -- host side of the L-SHADE / JADE / SaNSDE engine.
// Reference behaviour restated on the host: ShadeSearch::init/optimize/solution
// (shade.cpp:56-94, :238-256), JadeSearch likewise (jade.cpp:64-96, :208-226).
#include "bbo_de_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>

namespace bbo {

namespace {
enum { K_GEN = 0, K_BOOK, K_ARCH, K_RANK, K_FINISH, K_SELECT, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:de_generation", "bbo:de_bookkeep", "bbo:de_archive_copy", "bbo:de_rank", "bbo:de_finish", "bbo:de_select" };   // roctx ranges, bench.py's slot names
}

DeEngine::DeEngine(const bbo_params &p) :
        Engine(checked(p))
{
}

// the algorithm's own parameter checks, ahead of the base's (populations, device)
const bbo_params &DeEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_SHADE || p.algo == BBO_ALGO_JADE || p.algo == BBO_ALGO_SANSDE,
            "DeEngine: bad algo");
    if (p.algo == BBO_ALGO_SANSDE)
        BBO_REQUIRE(p.crref >= 1 && p.pupdate >= 1 && p.crupdate >= 1,
                "SANSDE: crref, pupdate, crupdate must be >= 1");
    BBO_REQUIRE(p.np >= 4, "DE needs a population of at least 4");
    if (p.algo == BBO_ALGO_SHADE) {
        BBO_REQUIRE(p.h >= 1, "SHADE: h must be >= 1");
        BBO_REQUIRE(p.npmin >= 4 && p.npmin <= p.np, "SHADE: need 4 <= npmin <= npinit");
    }
    return p;
}

void DeEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    (void) guess;   // JADE / SHADE never read it (jade.cpp:64-96, shade.cpp:56-94)
    BBO_REQUIRE(n >= 1 && n <= 2048, "DE: dimension must be in [1, 2048]");
    require_finite_box("DE draws its population from [lower, upper]: the bounds must be finite", n,
            lower, upper);
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations;
    DeConst &c = c_;
    c = DeConst {};
    c.variant = params_.algo == BBO_ALGO_SANSDE ? 2 : params_.algo == BBO_ALGO_JADE ? 1 : 0;
    c.ncrref = params_.crref;
    c.npup = params_.pupdate;
    c.ncrup = params_.crupdate;
    c.n = n;
    c.ld = round_up(n, 2);
    c.npinit = params_.np;
    c.npmin = c.variant == 0 ? params_.npmin : params_.np;
    c.h = c.variant == 0 ? params_.h : 1;
    c.archive = (params_.archive && c.variant != 2) ? 1 : 0;   // SaNSDE has no archive
    c.repaircr = params_.repaircr ? 1 : 0;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.tol = params_.tol;
    c.pelite = params_.pelite;
    c.cdamp = params_.cdamp;
    c.jsigma = params_.jade_sigma;
    c.seed = params_.seed;
    c.np_launch = c.npinit;

    const size_t rows = (size_t) P * c.npinit, ld = c.ld;
    Xa_.alloc(rows * ld);
    Xb_.alloc(rows * ld);
    fa_.alloc(rows);
    fb_.alloc(rows);
    arch_.alloc(c.variant == 2 ? 1 : rows * ld);
    cra_.alloc(rows);
    crb_.alloc(rows);
    MCR_.alloc((size_t) P * c.h);
    MF_.alloc((size_t) P * c.h);
    rec_cr_.alloc(rows);
    rec_f_.alloc(rows);
    rec_df_.alloc(rows);
    radius_.alloc(rows);
    order_.alloc(rows);
    rank_.alloc(rows);
    rec_flag_.alloc(rows);
    claim_.alloc(rows);
    slot_of_.alloc(rows);
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    std::vector<double> half((size_t) P * c.h, 0.5);
    MCR_.upload(half.data(), half.size());
    MF_.upload(half.data(), half.size());
    std::vector<DeScal> sc(P);
    for (auto &s : sc) {
        std::memset(&s, 0, sizeof(s));
        s.mucr = s.muf = 0.5;
        s.np = c.npinit;
        s.k = 1;
        s.fev = c.npinit;   // the initial population is evaluated (shade.cpp:88-89)
        s.sp = s.sfp = s.crm = 0.5;   // sansde.cpp:72-76
    }
    {
        std::vector<double> half_rows(rows, 0.5);   // sansde.cpp:90: every _cr starts at 0.5
        cra_.upload(half_rows.data(), rows);
        crb_.upload(half_rows.data(), rows);
    }
    scal_.upload(sc.data(), P);

    DeDev &d = d_;
    d = DeDev {};
    d.X[0] = Xa_.p; d.X[1] = Xb_.p; d.f[0] = fa_.p; d.f[1] = fb_.p;
    d.order = order_.p; d.rank = rank_.p; d.arch = arch_.p; d.MCR = MCR_.p; d.MF = MF_.p;
    d.rec_cr = rec_cr_.p; d.rec_f = rec_f_.p; d.rec_df = rec_df_.p; d.radius = radius_.p;
    d.rec_flag = rec_flag_.p; d.claim = claim_.p; d.slot_of = slot_of_.p;
    d.crow[0] = cra_.p; d.crow[1] = crb_.p;
    d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.scal = scal_.p;

    if (obj_.is_program()) prog_.bind(obj_.program, params_.device, n, P);
    else prog_.unbind();

    np_host_ = c.npinit;
    fev_host_ = c.npinit;
    c.honor_stop = 0;
    inited_ = true;

    const int R = rows_per_wg16(c.ld);
    dim3 grid((c.npinit + R - 1) / R, P);
    hipLaunchKernelGGL(de_init, grid, dim3(16 * R), (size_t) R * c.ld * sizeof(double), stream_,
            d_, c_);
    BBO_HIP(hipGetLastError());
    if (obj_.needs_host()) host_evaluate(0, c.npinit);
    else if (obj_.is_program()) program_evaluate(0, c.npinit);
    launch_rank(0, c.npinit);
    BBO_HIP(hipStreamSynchronize(stream_));
}

// ranks f[cur] (which_next = 0) or f[cur ^ 1] (1) of the first np individuals
void DeEngine::launch_rank(int which_next, int np_bound)
{
    const DeConst &c = c_;
    // (which form: rank_route, bbo_rank.hpp.  DE has the 8-slice counting kernel only, and its sort
    // always merges at 2048 / 4096 keys)
    last_rank_ = rank_route(np_bound, c.npop, RANK_DBG_COUNT32);
    switch (last_rank_) {
    case RK_WAVE:
        hipLaunchKernelGGL(de_rank_wave, dim3((c.npop + 3) / 4), dim3(256), 0, stream_, d_, c_,
                which_next);
        break;
    case RK_COUNT8: {
        dim3 rgrid((np_bound + 31) / 32, c.npop);
        hipLaunchKernelGGL(de_rank, rgrid, dim3(256), 0, stream_, d_, c_, which_next);
        break;
    }
    default: {
        const int m = rank_sort_m(np_bound);
        allow_lds((const void*) de_rank_sort, SORT_LDS_MAX * 12);
        // (2048 / 4096 keys: merge sort by merge path, two buffers; bbo_rank.hpp)
        hipLaunchKernelGGL(de_rank_sort, dim3(c.npop), dim3(sort_threads(m)),
                rank_sort_merges(m, 0) ? (size_t) m * 24 : (size_t) std::max(m, 1024) * 12,
                stream_, d_,
                c_, which_next, m);
        break;
    }
    }
    BBO_HIP(hipGetLastError());
}

// host objective: fitness of rows [0, rows) of buffer `which` of every population
void DeEngine::host_evaluate(int which, int rows)
{
    const DeConst &c = c_;
    BBO_HIP(hipStreamSynchronize(stream_));
    std::vector<DeScal> sc(c.npop);
    scal_.download(sc.data(), c.npop);
    std::vector<double> xh((size_t) rows * c.ld), fh(rows);
    for (int p = 0; p < c.npop; p++) {
        if (c.honor_stop && sc[p].stop) continue;
        const int buf = which < 0 ? (sc[p].cur ^ 1) : which;
        const int cnt = std::min(rows, sc[p].np);
        DevBuf<double> &X = buf == 0 ? Xa_ : Xb_;
        DevBuf<double> &F = buf == 0 ? fa_ : fb_;
        X.download(xh.data(), (size_t) cnt * c.ld, (size_t) p * c.npinit * c.ld);
        obj_.eval_host(xh.data(), cnt, c.n, c.ld, fh.data());
        nan_to_inf(fh.data(), cnt);
        F.upload(fh.data(), cnt, (size_t) p * c.npinit);
    }
}

// an objective program: the same rows, where they lie.  Which half holds them and how many are alive
// are device-side scalars: a small kernel writes the plan from them, the host reads nothing back.
void DeEngine::program_evaluate(int which, int rows)
{
    const DeConst &c = c_;
    const ProgScalView sv { d_.scal, (int) sizeof(DeScal), (int) offsetof(DeScal, cur), (int) offsetof(DeScal, np),
            (int) offsetof(DeScal, stop) };
    prog_.fill_plan(stream_, sv, Xa_.p, Xb_.p, fa_.p, fb_.p, c.npinit, c.ld, which, rows, c.honor_stop);
    prog_.launch(stream_, rows, nullptr, 0, &prog_timer_);
}

void DeEngine::generation(bool honor_stop)
{
    DeConst &c = c_;
    c.honor_stop = honor_stop ? 1 : 0;
    c.np_launch = np_host_;
    const int P = c.npop;
    dim3 g16((np_host_ + 15) / 16, P);
    const int R = rows_per_wg16(c.ld);     // rows staged in LDS per workgroup
    dim3 gR((np_host_ + R - 1) / R, P);
    const size_t lds = (size_t) R * c.ld * sizeof(double);
    const size_t lds_box = lds + (size_t) 2 * c.ld * sizeof(double);   // + lower, upper
    timed(K_GEN, [&] {
        if (c.variant == 2) {
            allow_lds((const void*) sansde_generation, 128 * 1024);
            hipLaunchKernelGGL(sansde_generation, gR, dim3(16 * R), lds_box, stream_, d_, c_);
        } else {
            allow_lds((const void*) de_generation, 128 * 1024);
            hipLaunchKernelGGL(de_generation, gR, dim3(16 * R), lds_box, stream_, d_, c_);
        }
    });
    if (!obj_.fused()) {
        if (obj_.is_program()) program_evaluate(-1, np_host_);
        else host_evaluate(-1, np_host_);
        timed(K_SELECT, [&] { hipLaunchKernelGGL(de_select, g16, dim3(256), 0, stream_, d_, c_); });
    }
    timed(K_BOOK, [&] {
        if (c.variant == 2)
            hipLaunchKernelGGL(sansde_bookkeep, dim3(P), dim3(pop_threads()), 0, stream_, d_, c_);
        else
            hipLaunchKernelGGL(de_bookkeep, dim3(P), dim3(pop_threads()), 0, stream_, d_, c_);
    });
    if (c.archive) {
        timed(K_ARCH, [&] { hipLaunchKernelGGL(de_archive_copy, g16, dim3(256), 0, stream_, d_, c_); });
    }
    timed(K_RANK, [&] { launch_rank(1, np_host_); });
    timed(K_FINISH, [&] { hipLaunchKernelGGL(de_finish, dim3(P), dim3(pop_threads()), 0, stream_, d_, c_); });
    // the same population-size schedule on the host (shade.cpp:218-225), for the grid only
    fev_host_ += np_host_;
    if (c.variant == 0) {
        const int npnew = (int) std::round((c.npmin - c.npinit) * ((1. * fev_host_) / c.mfev)
                + c.npinit);
        if (npnew < np_host_) np_host_ = std::max(npnew, c.npmin);
    }
}

void DeEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    DeScal s;
    scal_.download(&s, 1, population);
    int best = 0;
    order_.download(&best, 1, (size_t) population * c_.npinit);
    report_solution(s, s.cur == 0 ? Xa_ : Xb_, ((size_t) population * c_.npinit + best) * c_.ld, c_.n, c_.ld,
            x_out, n_evals, converged);
    if (s.gen == 0)     // converged() before any generation: the radius spread of the initial swarm
        *converged = radius_spread_converged(radius_, (size_t) population * c_.npinit, s.np, c_.tol);
}

int DeEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const DeConst &c = c_;
    DeScal s;
    scal_.download(&s, 1, p);
    const size_t pbase = (size_t) p * c.npinit;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    if (const int r = prog_get(k, out, cap); r >= 0) return r;
    // "x", "f" and "cr" (SaNSDE's per-individual CR) in sorted order, like the reference's _swarm
    if (k == "x") return o.rows_by_slot(s.cur == 0 ? Xa_ : Xb_, order_, pbase, s.np, c.npinit, c.n, c.ld);
    if (k == "f") return o.vec_by_slot(s.cur == 0 ? fa_ : fb_, order_, pbase, s.np, c.npinit);
    if (k == "cr") return o.vec_by_slot(s.cur == 0 ? cra_ : crb_, order_, pbase, s.np, c.npinit);
    if (k == "arch") return o.rows(arch_, pbase, s.larch, c.n, c.ld);
    if (k == "MCR" || k == "MF") return o.vec(k == "MCR" ? MCR_ : MF_, (size_t) p * c.h, c.h);
    if (k == "rec_flag") return o.ints(rec_flag_, pbase, s.np);
    if (k == "rec_cr" || k == "rec_f" || k == "rec_df")
        return o.vec(k == "rec_cr" ? rec_cr_ : k == "rec_f" ? rec_f_ : rec_df_, pbase, s.np);
    if (k == "pns" || k == "pnf" || k == "fpns" || k == "fpnf") {
        if (out && cap >= 2)
            for (int q = 0; q < 2; q++)
                out[q] = k == "pns" ? s.pns[q] : k == "pnf" ? s.pnf[q] : k == "fpns" ? s.fpns[q]
                                                                                     : s.fpnf[q];
        return 2;
    }
    if (k == "p") return o.one(s.sp);
    if (k == "fp") return o.one(s.sfp);
    if (k == "crm") return o.one(s.crm);
    if (k == "crrec") return o.one(s.crrec);
    if (k == "crdeltaf") return o.one(s.crdeltaf);
    if (k == "it") return o.one(s.gen);
    if (k == "k") return o.one(s.k);
    if (k == "np") return o.one(s.np);
    if (k == "fev") return o.one(s.fev);
    if (k == "gen") return o.one(s.gen);
    if (k == "larch") return o.one(s.larch);
    if (k == "mucr") return o.one(s.mucr);
    if (k == "muf") return o.one(s.muf);
    if (k == "stop") return o.one(s.stop);
    if (k == "conv") return o.one(s.conv);
    if (k == "m2") return o.one(s.m2);
    if (k == "nsucc") return o.one(s.nsucc);
    if (k == "n") return o.one(c.n);
    if (k == "rank_route") return o.one(last_rank_);     // the form of the last launch_rank: RankKernel
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int DeEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    const DeConst &c = c_;
    DeScal s;
    scal_.download(&s, 1, p);
    const size_t pbase = (size_t) p * c.npinit;
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (const int r = prog_set(k, in, count); r >= 0) return r;
    if (k == "x") {   // rows in sorted order; follow with set("f") to re-rank
        BBO_REQUIRE(count % c.n == 0 && count / c.n <= c.npinit, "set x: bad element count");
        const int rows = count / c.n;
        upload_rows(s.cur == 0 ? Xa_ : Xb_, pbase, rows, c.n, c.ld, in);
        s.np = rows;
        scal_.upload(&s, 1, p);
        np_host_ = std::max(np_host_, rows);
        return count;
    }
    if (k == "f") {
        BBO_REQUIRE(count == s.np, "set f: count must equal np");
        (s.cur == 0 ? fa_ : fb_).upload(in, count, pbase);
        c_.honor_stop = 0;
        c_.np_launch = c.npinit;
        launch_rank(0, c.npinit);
        BBO_HIP(hipStreamSynchronize(stream_));
        return count;
    }
    if (k == "arch") {
        BBO_REQUIRE(count % c.n == 0 && count / c.n <= c.npinit, "set arch: bad element count");
        const int rows = count / c.n;
        if (rows > 0) upload_rows(arch_, pbase, rows, c.n, c.ld, in);
        s.larch = rows;
        scal_.upload(&s, 1, p);
        return count;
    }
    if (k == "MCR" || k == "MF") {
        BBO_REQUIRE(count == c.h, "set MCR/MF: count must equal h");
        (k == "MCR" ? MCR_ : MF_).upload(in, c.h, (size_t) p * c.h);
        return count;
    }
    BBO_REQUIRE(count == 1, "set: wrong element count");
    if (k == "k") s.k = (int) in[0];
    else if (k == "fev") { s.fev = (int) in[0]; fev_host_ = s.fev; }
    else if (k == "gen") s.gen = (int) in[0];
    else if (k == "mucr") s.mucr = in[0];
    else if (k == "muf") s.muf = in[0];
    else if (k == "stop") s.stop = (int) in[0];
    else throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
    scal_.upload(&s, 1, p);
    return 1;
}

Optimizer* make_de_engine(const bbo_params &p)
{
    return new DeEngine(p);
}

} // namespace bbo
