// bbo_mayfly.hip -- host side of the mayfly engine.  Reference behaviour restated on the host:
// MayflySearch::MayflySearch / init / optimize / solution (mayfly.cpp:39-163, :284-295).
#include "bbo_mayfly_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_INIT = 0, K_BEGIN, K_FEMALES, K_MALES, K_RANK, K_CROSS, K_MUTATE, K_MERGE, K_RESOLVE, K_COPY, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:mayfly_init", "bbo:mayfly_begin", "bbo:mayfly_females",
        "bbo:mayfly_males", "bbo:mayfly_rank", "bbo:mayfly_cross", "bbo:mayfly_mutate", "bbo:mayfly_merge",
        "bbo:mayfly_resolve", "bbo:mayfly_copy" };
}

MayflyEngine::MayflyEngine(const bbo_params &p) :
        Engine(checked(p))
{
    bbo_mayfly_params_default(&mp_);
}

// the part of the constructor's arguments that travels in bbo_params
const bbo_params &MayflyEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_MAYFLY, "MayflyEngine: bad algo");
    BBO_REQUIRE(p.np >= 2 && p.np <= MAYFLY_MAX_NP, "Mayfly: np must be in [2, 4096]");
    BBO_REQUIRE(p.np % 2 == 0, "Mayfly: np must be even (the reference leaves the last offspring of an odd swarm "
            "unwritten: a zero vector of value 0 that enters the selection)");
    BBO_REQUIRE(p.mfev > 2 * p.np, "Mayfly: mfev must exceed 2 np (the initial swarms alone cost 2 np evaluations; "
            "itmax would be <= 0 and g = 0/0)");
    return p;
}

void MayflyEngine::configure(const bbo_mayfly_params &mp)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_mayfly_configure after bbo_init");
    const double vals[] = { mp.a1, mp.a2, mp.a3, mp.beta, mp.dance, mp.ddamp, mp.fl, mp.fldamp, mp.gmin, mp.gmax,
            mp.vdamp, mp.sigma, mp.pmutdim, mp.pmutnp, mp.l };
    for (double v : vals) BBO_REQUIRE(std::isfinite(v), "Mayfly: every parameter must be finite");
    BBO_REQUIRE(mp.pmutdim >= 0. && mp.pmutdim <= 1., "Mayfly: pmutdim must lie in [0, 1]");
    BBO_REQUIRE(mp.pmutnp >= 0. && mp.pmutnp <= 1., "Mayfly: pmutnp must lie in [0, 1]");
    BBO_REQUIRE(mp.vdamp >= 0., "Mayfly: vdamp must not be negative");
    BBO_REQUIRE(mp.pgb == 0 || mp.pgb == 1, "Mayfly: pgb is 0 or 1");
    BBO_REQUIRE(mp.repair == 0 || mp.repair == 1, "Mayfly: repair is 0 or 1");
    BBO_REQUIRE(mp.substream >= 0 && mp.substream < (1 << 24), "Mayfly: substream must be in [0, 2^24)");
    mp_ = mp;
}

// the pointers the kernels take: the swarms in buffer cur_, the selection's target in the other
void MayflyEngine::bind()
{
    MayflyDev &d = d_;
    const int a = cur_, b = 1 - cur_;
    d.MX = MX_[a].p; d.MV = MV_[a].p; d.MBX = MBX_[a].p; d.Mf = Mf_[a].p; d.Mbf = Mbf_[a].p;
    d.FX = FX_[a].p; d.FV = FV_[a].p; d.Ff = Ff_[a].p;
    d.MX2 = MX_[b].p; d.MV2 = MV_[b].p; d.MBX2 = MBX_[b].p; d.Mf2 = Mf_[b].p; d.Mbf2 = Mbf_[b].p;
    d.FX2 = FX_[b].p; d.FV2 = FV_[b].p; d.Ff2 = Ff_[b].p;
}

// the candidate rows of a round of the male loop
void MayflyEngine::alloc_window()
{
    const int W = window_ == 0 ? c_.np : std::min(window_, c_.np);
    c_.window = W;
    candx_.alloc((size_t) c_.npop * W * c_.ld);
    candv_.alloc((size_t) c_.npop * W * c_.ld);
    candf_.alloc((size_t) c_.npop * W);
    d_.candx = candx_.p; d_.candv = candv_.p; d_.candf = candf_.p;
}

void MayflyEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    (void) guess;   // the reference never reads it (mayfly.cpp:63-163)
    reject_program(obj, "Mayfly");
    BBO_REQUIRE(n >= 1 && n <= MAYFLY_MAX_N, "Mayfly: dimension must be in [1, 512]");
    require_finite_box("Mayfly draws its swarms from [lower, upper] and scales its velocities by the box: the bounds must be finite",
            n, lower, upper);
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations, np = params_.np;
    BBO_REQUIRE(P <= (1 << 24), "Mayfly: populations must be <= 2^24");
    MayflyConst &c = c_;
    c = MayflyConst {};
    c.n = n;
    c.ld = round_up(n, 2);
    c.np = np;
    // :135-139
    c.nmut = (int) (mp_.pmutnp * np);
    if (c.nmut % 2 != 0) c.nmut = std::min(c.nmut + 1, np);
    c.nmd = (int) std::ceil(mp_.pmutdim * n);
    c.cm = np + np / 2 + c.nmut / 2;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.pgb = mp_.pgb;
    c.repair = mp_.repair;
    c.sub0 = mp_.substream;
    c.kb_np = shuffle_key_bits(np);
    c.kb_nmut = shuffle_key_bits(std::max(c.nmut, 1));
    c.kb_n = shuffle_key_bits(n);
    c.table = (int) mayfly_table(n, np, c.nmut, c.nmd).len;
    c.a1 = mp_.a1; c.a2 = mp_.a2; c.a3 = mp_.a3; c.beta = mp_.beta; c.ddamp = mp_.ddamp; c.fldamp = mp_.fldamp;
    c.gmin = mp_.gmin; c.gmax = mp_.gmax; c.vdamp = mp_.vdamp; c.sigma = mp_.sigma; c.l = mp_.l;
    c.seed = params_.seed;

    const size_t rows = (size_t) P * np, mrows = (size_t) P * c.nmut;
    for (int b = 0; b < 2; b++) {
        MX_[b].alloc(rows * c.ld); MV_[b].alloc(rows * c.ld); MBX_[b].alloc(rows * c.ld);
        Mf_[b].alloc(rows); Mbf_[b].alloc(rows);
        FX_[b].alloc(rows * c.ld); FV_[b].alloc(rows * c.ld); Ff_[b].alloc(rows);
    }
    OX_.alloc(rows * c.ld); Of_.alloc(rows);
    UX_.alloc(mrows * c.ld); Uf_.alloc(mrows);
    best_.alloc((size_t) P * c.ld);
    keys_.alloc((size_t) P * 2 * c.cm);
    ordm_.alloc(rows); ordf_.alloc(rows); ordt_.alloc((size_t) P * 2 * c.cm);
    srcm_.alloc(rows); srcf_.alloc(rows); permo_.alloc(rows); permu_.alloc(mrows);
    brm_.alloc(rows); brf_.alloc(rows);
    tables_.clear();
    record_ = false;
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    {
        std::vector<MayflyScal> sc(P);
        std::memset(sc.data(), 0, sizeof(MayflyScal) * P);
        for (auto &s : sc) {
            s.fev = np + np;                // :132
            s.itmax = (int) std::ceil((params_.mfev - s.fev) / (3. * np + c.nmut));     // :159
            s.g = mp_.gmax;
            s.dance = mp_.dance;
            s.fl = mp_.fl;
            s.took = -1;
            s.fbest = std::numeric_limits<double>::infinity();
        }
        scal_.upload(sc.data(), P);
        std::vector<int> id(rows);
        for (size_t r = 0; r < rows; r++) id[r] = (int) (r % np);
        ordm_.upload(id.data(), rows);
        ordf_.upload(id.data(), rows);
        srcm_.upload(id.data(), rows);
        srcf_.upload(id.data(), rows);
        permo_.upload(id.data(), rows);
    }

    cur_ = 0;
    MayflyDev &d = d_;
    d = MayflyDev {};
    bind();
    d.OX = OX_.p; d.Of = Of_.p; d.UX = UX_.p; d.Uf = Uf_.p; d.best = best_.p; d.keys = keys_.p;
    d.ordm = ordm_.p; d.ordf = ordf_.p; d.ordt = ordt_.p; d.srcm = srcm_.p; d.srcf = srcf_.p;
    d.permo = permo_.p; d.permu = permu_.p; d.brm = brm_.p; d.brf = brf_.p;
    d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.scal = scal_.p;
    alloc_window();
    inited_ = true;

    const dim3 grid(P, (np + MAYFLY_INIT_ROWS - 1) / MAYFLY_INIT_ROWS, 2);
    const int mode = MAYFLY_INIT_DRAW | (obj_.needs_host() ? 0 : MAYFLY_INIT_EVAL);
    timed(K_INIT, [&] { hipLaunchKernelGGL(mayfly_init, grid, dim3(256), 0, stream_, d_, c_, 0, mode); });
    if (obj_.needs_host()) host_evaluate_init();
    timed(K_INIT, [&] { hipLaunchKernelGGL(mayfly_init_best, dim3(P), dim3(64), 0, stream_, d_, c_, 0); });
    BBO_HIP(hipStreamSynchronize(stream_));
}

// host objective: male j, then female j (:81-131)
void MayflyEngine::host_evaluate_init()
{
    BBO_HIP(hipStreamSynchronize(stream_));
    const int np = c_.np, ld = c_.ld;
    std::vector<double> xm((size_t) np * ld), xf((size_t) np * ld), fm(np), ff(np);
    for (int p = 0; p < c_.npop; p++) {
        // (the points drawn: the reference stores them as the velocities, kernels header)
        (c_.repair ? MX_ : MV_)[cur_].download(xm.data(), xm.size(), (size_t) p * np * ld);
        (c_.repair ? FX_ : FV_)[cur_].download(xf.data(), xf.size(), (size_t) p * np * ld);
        for (int j = 0; j < np; j++) {
            obj_.eval_host(xm.data() + (size_t) j * ld, 1, c_.n, ld, &fm[j]);
            obj_.eval_host(xf.data() + (size_t) j * ld, 1, c_.n, ld, &ff[j]);
        }
        nan_to_inf(fm.data(), np);
        nan_to_inf(ff.data(), np);
        Mf_[cur_].upload(fm.data(), np, (size_t) p * np);
        Ff_[cur_].upload(ff.data(), np, (size_t) p * np);
    }
}

// host objective: the male loop one male at a time, so that the callable sees no male that is dropped
void MayflyEngine::host_male_loop(bool honor_stop)
{
    const int P = c_.npop, ld = c_.ld;
    std::vector<MayflyScal> sc(P);
    std::vector<double> x(ld);
    for (int j = 0; j < c_.np; j++) {
        timed(K_MALES, [&] { hipLaunchKernelGGL(mayfly_males, dim3(P), dim3(MAYFLY_WG), 0, stream_, d_, c_, (int) MAYFLY_FORM); });
        BBO_HIP(hipStreamSynchronize(stream_));
        if (j == 0) scal_.download(sc.data(), P);
        for (int p = 0; p < P; p++) {
            if (honor_stop && sc[p].stop) continue;
            candx_.download(x.data(), ld, (size_t) p * c_.window * ld);
            double f = 0.;
            obj_.eval_host(x.data(), 1, c_.n, ld, &f);
            nan_to_inf(&f, 1);
            candf_.upload(&f, 1, (size_t) p * c_.window);
        }
        timed(K_MALES, [&] { hipLaunchKernelGGL(mayfly_males, dim3(P), dim3(MAYFLY_WG), 0, stream_, d_, c_, (int) MAYFLY_ABSORB); });
    }
}

void MayflyEngine::launch_rank(int which, int count)
{
    const dim3 grid(c_.npop, (count + MAYFLY_RANK_CANDS - 1) / MAYFLY_RANK_CANDS, 2);
    timed(K_RANK, [&] { hipLaunchKernelGGL(mayfly_rank, grid, dim3(256), 0, stream_, d_, c_, which); });
}

// one iterate() of the reference in every population (:165-282)
void MayflyEngine::generation(bool honor_stop)
{
    c_.honor_stop = honor_stop ? 1 : 0;
    const bool host = obj_.needs_host();
    const int P = c_.npop, np = c_.np, n = c_.n, ld = c_.ld;
    timed(K_BEGIN, [&] { hipLaunchKernelGGL(mayfly_begin, dim3(P), dim3(256), 0, stream_, d_, c_); });
    timed(K_FEMALES, [&] { hipLaunchKernelGGL(mayfly_females, dim3(np, P), dim3(64), 0, stream_, d_, c_); });
    if (host) {
        host_evaluate_rows(FX_[cur_], Ff_[cur_], np, n, ld, honor_stop);
        host_male_loop(honor_stop);
    } else {
        timed(K_MALES, [&] { hipLaunchKernelGGL(mayfly_males, dim3(P), dim3(MAYFLY_WG), 0, stream_, d_, c_, (int) MAYFLY_FUSED); });
    }
    launch_rank(0, np);
    timed(K_CROSS, [&] { hipLaunchKernelGGL(mayfly_cross, dim3(np, P), dim3(64), 0, stream_, d_, c_); });
    if (host) host_evaluate_rows(OX_, Of_, np, n, ld, honor_stop);
    if (c_.nmut > 0) {
        timed(K_MUTATE, [&] { hipLaunchKernelGGL(mayfly_mutate, dim3(c_.nmut, P), dim3(64), 0, stream_, d_, c_); });
        if (host) host_evaluate_rows(UX_, Uf_, c_.nmut, n, ld, honor_stop);
    }
    timed(K_MERGE, [&] { hipLaunchKernelGGL(mayfly_merge, dim3(P), dim3(256), 0, stream_, d_, c_); });
    launch_rank(1, c_.cm);
    timed(K_RESOLVE, [&] { hipLaunchKernelGGL(mayfly_resolve, dim3(P), dim3(128), 0, stream_, d_, c_); });
    timed(K_COPY, [&] { hipLaunchKernelGGL(mayfly_copy, dim3(np, P, 2), dim3(64), 0, stream_, d_, c_); });
    cur_ = 1 - cur_;
    bind();
}

void MayflyEngine::inject_draws(const double *table, int count)
{
    enter("bbo_mayfly_inject_draws");
    BBO_HIP(hipStreamSynchronize(stream_));
    if (!table) {
        d_.inject = nullptr;
        return;
    }
    const int P = c_.npop, n = c_.n, np = c_.np, nmut = c_.nmut, nmd = c_.nmd;
    const MayflyTable t = mayfly_table(n, np, nmut, nmd);
    BBO_REQUIRE(count > 0 && (size_t) count == (size_t) P * t.len,
            "bbo_mayfly_inject_draws: populations * (2 np n + np + nmut + 2 nmut nmd) values");
    for (int p = 0; p < P; p++) {
        const double *tb = table + (size_t) p * t.len;
        for (size_t q = 0; q < t.po; q++)
            BBO_REQUIRE(tb[q] == -1. || (tb[q] >= 0. && tb[q] < 1.),
                    "bbo_mayfly_inject_draws: uniforms lie in [0, 1), -1 where none is drawn");
        permutation_of(tb + t.po, np, "bbo_mayfly_inject_draws: the offspring shuffle is a permutation of 0 .. np - 1");
        permutation_of(tb + t.pu, nmut, "bbo_mayfly_inject_draws: the shuffle of the mutated flies is a permutation of 0 .. nmut - 1");
        for (int u = 0; u < nmut; u++) {
            std::vector<char> seen(n, 0);
            for (int q = 0; q < nmd; q++) {
                const double k = tb[t.ix + (size_t) u * nmd + q], z = tb[t.z + (size_t) u * nmd + q];
                BBO_REQUIRE(k >= 0. && k < n && k == std::floor(k) && !seen[(int) k],
                        "bbo_mayfly_inject_draws: the genes of a mutated fly are distinct integers in [0, n)");
                seen[(int) k] = 1;
                BBO_REQUIRE(std::isfinite(z), "bbo_mayfly_inject_draws: normals must be finite");
            }
        }
    }
    d_.inject = tables_.load(table, (size_t) P * t.len);
}

void MayflyEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    MayflyScal s;
    scal_.download(&s, 1, population);
    s.conv = 0;     // :284-286: never converged
    report_solution(s, best_, (size_t) population * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

int MayflyEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const MayflyConst &c = c_;
    MayflyScal s;
    scal_.download(&s, 1, p);
    const size_t pr = (size_t) p * c.np;
    const StateOut o { out, cap };
    const int a = cur_;
    if (k == "profile") return profile_report(out, cap);
    if (k == "males_x") return o.rows(MX_[a], pr, c.np, c.n, c.ld);
    if (k == "males_v") return o.rows(MV_[a], pr, c.np, c.n, c.ld);
    if (k == "males_bx") return o.rows(MBX_[a], pr, c.np, c.n, c.ld);
    if (k == "males_f") return o.vec(Mf_[a], pr, c.np);
    if (k == "males_bf") return o.vec(Mbf_[a], pr, c.np);
    if (k == "females_x") return o.rows(FX_[a], pr, c.np, c.n, c.ld);
    if (k == "females_v") return o.rows(FV_[a], pr, c.np, c.n, c.ld);
    if (k == "females_f") return o.vec(Ff_[a], pr, c.np);
    // what the last generation worked on, in the buffer it left behind
    if (k == "moved_males_x") return o.rows(MX_[1 - a], pr, c.np, c.n, c.ld);
    if (k == "moved_males_v") return o.rows(MV_[1 - a], pr, c.np, c.n, c.ld);
    if (k == "moved_males_f") return o.vec(Mf_[1 - a], pr, c.np);
    if (k == "moved_females_x") return o.rows(FX_[1 - a], pr, c.np, c.n, c.ld);
    if (k == "moved_females_v") return o.rows(FV_[1 - a], pr, c.np, c.n, c.ld);
    if (k == "moved_females_f") return o.vec(Ff_[1 - a], pr, c.np);
    if (k == "off_x") return o.rows(OX_, pr, c.np, c.n, c.ld);
    if (k == "off_f") return o.vec(Of_, pr, c.np);
    if (k == "mut_x") return o.rows(UX_, (size_t) p * c.nmut, c.nmut, c.n, c.ld);
    if (k == "mut_f") return o.vec(Uf_, (size_t) p * c.nmut, c.nmut);
    if (k == "xbest") return o.vec(best_, (size_t) p * c.ld, c.n);
    if (k == "rank_m") return o.ints(ordm_, pr, c.np);
    if (k == "rank_f") return o.ints(ordf_, pr, c.np);
    if (k == "sel_m") return o.ints(ordt_, (size_t) p * 2 * c.cm, c.cm);
    if (k == "sel_f") return o.ints(ordt_, ((size_t) p * 2 + 1) * c.cm, c.cm);
    if (k == "src_m") return o.ints(srcm_, pr, c.np);
    if (k == "src_f") return o.ints(srcf_, pr, c.np);
    if (k == "branch_m") return o.ints(brm_, pr, c.np);
    if (k == "branch_f") return o.ints(brf_, pr, c.np);
    if (k == "perm_o") return o.ints(permo_, pr, c.np);
    if (k == "perm_u") return o.ints(permu_, (size_t) p * c.nmut, c.nmut);
    if (k == "draws") {
        require_record(record_, k);
        return o.vec(tables_.draws, (size_t) p * c.table, c.table);
    }
    if (k == "fbest") return o.one(s.fbest);
    if (k == "g") return o.one(s.g);
    if (k == "dance") return o.one(s.dance);
    if (k == "fl") return o.one(s.fl);
    if (k == "it") return o.one(s.it);
    if (k == "itmax") return o.one(s.itmax);
    if (k == "fev") return o.one(s.fev);
    if (k == "nmut") return o.one(c.nmut);
    if (k == "nmd") return o.one(c.nmd);
    if (k == "took") return o.one(s.took);
    if (k == "dropped") return o.one(s.dropped);
    if (k == "rounds") return o.one(s.rounds);
    if (k == "flag" || k == "stop") return o.one(s.stop);
    if (k == "conv") return o.one(0.);
    if (k == "window") return o.one(window_);
    if (k == "record_draws") return o.one(record_ ? 1. : 0.);
    if (k == "table_len") return o.one(c.table);
    if (k == "repair") return o.one(c.repair);
    if (k == "substream") return o.one(c.sub0);
    if (k == "pgb") return o.one(c.pgb);
    if (k == "np") return o.one(c.np);
    if (k == "n") return o.one(c.n);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int MayflyEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    const MayflyConst &c = c_;
    const size_t pr = (size_t) p * c.np;
    const int a = cur_;
    auto whole = [&](double lo, double hi) {
        return count == 1 && in[0] == std::floor(in[0]) && in[0] >= lo && in[0] <= hi;
    };
    auto rows = [&](DevBuf<double> &b) {
        BBO_REQUIRE(count == c.np * c.n, k + ": np * n values");
        upload_rows(b, pr, c.np, c.n, c.ld, in);
        return count;
    };
    auto vals = [&](DevBuf<double> &b) {
        BBO_REQUIRE(count == c.np, k + ": np values");
        std::vector<double> fh(in, in + count);
        nan_to_inf(fh.data(), count);
        b.upload(fh.data(), c.np, pr);
        return count;
    };
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "record_draws") {      // (the whole handle) the draws of the last generation in the layout of inject_draws
        BBO_REQUIRE(whole(0., 1.), "record_draws: 0 or 1");
        record_ = in[0] != 0.;
        d_.draws = tables_.record(record_, (size_t) c.npop * c.table);
        return 1;
    }
    if (k == "window") {            // (the whole handle) males per round of the male loop; 0: all remaining
        BBO_REQUIRE(whole(0., (double) MAYFLY_MAX_NP), "window: 0 (all remaining males) or the males of a round, up to 4096");
        window_ = (int) in[0];
        alloc_window();
        return 1;
    }
    // a whole state, key by key: nothing is evaluated and nothing follows from what is written
    if (k == "males_x") return rows(MX_[a]);
    if (k == "males_v") return rows(MV_[a]);
    if (k == "males_bx") return rows(MBX_[a]);
    if (k == "males_f") return vals(Mf_[a]);
    if (k == "males_bf") return vals(Mbf_[a]);
    if (k == "females_x") return rows(FX_[a]);
    if (k == "females_v") return rows(FV_[a]);
    if (k == "females_f") return vals(Ff_[a]);
    if (k == "xbest") {
        BBO_REQUIRE(count == c.n, "xbest: n values");
        std::vector<double> x(c.ld, 0.);
        std::copy(in, in + c.n, x.begin());
        best_.upload(x.data(), c.ld, (size_t) p * c.ld);
        return count;
    }
    MayflyScal s;
    scal_.download(&s, 1, p);
    if (k == "fbest" || k == "g" || k == "dance" || k == "fl") {
        BBO_REQUIRE(count == 1 && in[0] == in[0], k + ": one value, not NaN");
        (k == "fbest" ? s.fbest : k == "g" ? s.g : k == "dance" ? s.dance : s.fl) = in[0];
    } else if (k == "fev" || k == "it") {       // (the budget test looks at fev after the next generation)
        BBO_REQUIRE(whole(0., 2147483646.), "fev, it: one non-negative integer");
        (k == "fev" ? s.fev : s.it) = (int) in[0];
    } else if (k == "itmax") {
        BBO_REQUIRE(whole(1., 2147483646.), "itmax: one positive integer");
        s.itmax = (int) in[0];
    } else {
        throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
    }
    scal_.upload(&s, 1, p);
    return 1;
}

Optimizer* make_mayfly_engine(const bbo_params &p)
{
    return new MayflyEngine(p);
}

} // namespace bbo
