// bbo_cso.hip -- host side of the CSO engine.  Reference behaviour restated on the host:
// CSOSearch::CSOSearch / init / optimize / solution (cso.cpp:46-112, :160-175).
#include "bbo_cso_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>

namespace bbo {

namespace {
enum { K_MEAN = 0, K_SHUFFLE, K_GROUPS, K_COMPETE, K_FINISH, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:cso_mean", "bbo:cso_shuffle", "bbo:cso_groups", "bbo:cso_compete", "bbo:cso_finish" };   // roctx ranges, bench.py's slot names
}

CsoEngine::CsoEngine(const bbo_params &p) :
        Engine(checked(p))
{
}

// the algorithm's own parameter checks and adjustments, ahead of the base's (populations, device)
bbo_params CsoEngine::checked(bbo_params p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_CSO, "CsoEngine: bad algo");
    BBO_REQUIRE(p.np >= 2, "CSO needs at least 2 particles");
    // cso.cpp:53-64: at least two particles per competition, np rounded up to a multiple
    if (p.pcompete < 2) {
        p.pcompete = 2;
        fprintf(stderr, "Warning [CSO]: particles per competition is too small - adjusted.\n");
    }
    while (p.np % p.pcompete != 0) p.np++;
    return p;
}

void CsoEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    (void) guess;   // CSO never reads it (cso.cpp:67-112)
    reject_program(obj, "CSO");
    BBO_REQUIRE(n >= 1 && n <= 1024, "CSO: dimension must be in [1, 1024]");
    require_finite_box("CSO draws its swarm from [lower, upper]: the bounds must be finite", n,
            lower, upper);
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations;
    CsoConst &c = c_;
    c = CsoConst {};
    c.n = n;
    c.ld = round_up(n, 2);
    c.np = params_.np;
    c.pc = params_.pcompete;
    c.ngroup = c.np / c.pc;
    c.ring = params_.ring ? 1 : 0;
    c.correct = params_.correct ? 1 : 0;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.stol = params_.tol;
    c.vmax = params_.vmax;
    c.seed = params_.seed;
    c.parts = std::max(1, std::min(256, c.np / 64));
    c.fparts = std::max(1, std::min(64, c.np / 1024));
    // cso.cpp:196-217
    if (c.pc == 2) {
        if (c.np <= 100) {
            c.phil = c.phih = 0.;
        } else {
            c.phil = std::max(0., 0.14 * std::log(c.np) - 0.3);
            c.phih = std::max(0., 0.27 * std::log(c.np) - 0.51);
        }
    } else {
        c.phil = 0.;
        c.phih = 0.3;
    }

    const size_t rows = (size_t) P * c.np, ld = c.ld;
    X_.alloc(rows * ld);
    V_.alloc(rows * ld);
    PM_.alloc(c.ring ? rows * ld : 1);
    f_.alloc(rows);
    radius_.alloc(rows);
    occ_.alloc(rows);
    occ2_.alloc(rows);
    mean_.alloc(P * ld);
    meanw_.alloc(P * ld);
    colpart_.alloc((size_t) P * c.parts * ld);
    // the swarm mean from cso_compete's own sums where a lane's share of a row is at most four
    // column pairs (ld <= 512 with up to 64 lanes per group) and the global mean is what is used
    fuse_g_ = (c.ring || c.ld > 512) ? 0 : c.ld <= 128 ? 16 : c.ld <= 256 ? 32 : 64;
    c.nwg = fuse_g_ ? (c.ngroup + 256 / fuse_g_ - 1) / (256 / fuse_g_) : 1;
    wgpart_.alloc(fuse_g_ ? (size_t) P * c.nwg * ld : 1);
    fpart_.alloc((size_t) P * c.fparts * CSO_FPART);
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    std::vector<CsoScal> sc(P);
    for (auto &s : sc) {
        std::memset(&s, 0, sizeof(s));
        s.fev = c.np;          // the initial swarm is evaluated (cso.cpp:99)
        s.fbest = std::numeric_limits<double>::infinity();
    }
    scal_.upload(sc.data(), P);

    CsoDev &d = d_;
    d = CsoDev {};
    d.X = X_.p; d.V = V_.p; d.PM = PM_.p; d.f = f_.p; d.radius = radius_.p;
    d.occ = occ_.p; d.occ2 = occ2_.p;
    d.mean = mean_.p; d.meanw = meanw_.p; d.colpart = colpart_.p; d.fpart = fpart_.p;
    d.wgpart = wgpart_.p;
    d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.scal = scal_.p;
    c.honor_stop = 0;
    inited_ = true;

    const int R = rows_per_wg16(c.ld);
    hipLaunchKernelGGL(cso_init, dim3((c.np + R - 1) / R, P), dim3(16 * R),
            (size_t) R * c.ld * sizeof(double), stream_, d_, c_);
    BBO_HIP(hipGetLastError());
    if (obj_.needs_host()) host_evaluate(false);
    hipLaunchKernelGGL(cso_finish_part, dim3(c_.fparts, P), dim3(256), 0, stream_, d_, c_);
    hipLaunchKernelGGL(cso_finish, dim3(P), dim3(64), 0, stream_, d_, c_, 1);
    if (fuse_g_) {      // the sums cso_compete maintains from now on, of the initial swarm
        const size_t lds = (size_t) (256 / fuse_g_ + 2) * c.ld * sizeof(double);   // rows + the box
        const dim3 grid(c.nwg, P);
        if (fuse_g_ == 16) hipLaunchKernelGGL(cso_team_colsum<16>, grid, dim3(256), lds, stream_, d_, c_);
        else if (fuse_g_ == 32) hipLaunchKernelGGL(cso_team_colsum<32>, grid, dim3(256), lds, stream_, d_, c_);
        else hipLaunchKernelGGL(cso_team_colsum<64>, grid, dim3(256), lds, stream_, d_, c_);
    }
    BBO_HIP(hipGetLastError());
    BBO_HIP(hipStreamSynchronize(stream_));
}

// host objective: every particle (init) or the losers of this generation (slots that are not
// the first of their group: the winner of a group does not move), in slot order
void CsoEngine::host_evaluate(bool losers_only)
{
    const int pc = c_.pc;
    host_evaluate_rows(X_, f_, c_.np, c_.n, c_.ld, c_.honor_stop, &occ_,
            [=](int s) { return losers_only && s % pc == 0; });
}

void CsoEngine::generation(bool honor_stop)
{
    CsoConst &c = c_;
    c.honor_stop = honor_stop ? 1 : 0;
    const int P = c.npop;
    timed(K_MEAN, [&] {
        if (c.ring) {
            hipLaunchKernelGGL(cso_ring_mean, dim3((c.np + 15) / 16, P), dim3(256), 0, stream_, d_, c_);
        } else if (fuse_g_) {
            hipLaunchKernelGGL(cso_wgsum, dim3(c.parts, P), dim3(256), 0, stream_, d_, c_);
            hipLaunchKernelGGL(cso_mean, dim3(P), dim3(256), 0, stream_, d_, c_, 0, c.np);
        } else {
            hipLaunchKernelGGL(cso_colsum, dim3(c.parts, P), dim3(256), 0, stream_, d_, c_, 1, c.np);
            hipLaunchKernelGGL(cso_mean, dim3(P), dim3(256), 0, stream_, d_, c_, 0, c.np);
        }
    });
    timed(K_SHUFFLE, [&] {
        hipLaunchKernelGGL(cso_shuffle, dim3((c.np + 255) / 256, P), dim3(256), 0, stream_, d_, c_,
                shuffle_key_bits(c.np));
    });
    timed(K_GROUPS, [&] {
        hipLaunchKernelGGL(cso_groups, dim3((c.ngroup + 255) / 256, P), dim3(256), 0, stream_, d_, c_);
        hipLaunchKernelGGL(cso_colsum, dim3(c.parts, P), dim3(256), 0, stream_, d_, c_, c.pc,
                c.ngroup);
        hipLaunchKernelGGL(cso_mean, dim3(P), dim3(256), 0, stream_, d_, c_, 1, c.ngroup);
    });
    timed(K_COMPETE, [&] {
        if (fuse_g_) {
            const size_t lds = (size_t) (256 / fuse_g_ + 2) * c.ld * sizeof(double);   // rows + the box
            const dim3 grid(c.nwg, P);
            if (fuse_g_ == 16)
                hipLaunchKernelGGL((cso_compete<16, true>), grid, dim3(256), lds, stream_, d_, c_);
            else if (fuse_g_ == 32)
                hipLaunchKernelGGL((cso_compete<32, true>), grid, dim3(256), lds, stream_, d_, c_);
            else
                hipLaunchKernelGGL((cso_compete<64, true>), grid, dim3(256), lds, stream_, d_, c_);
        } else {
            const int R = rows_per_wg16(c.ld);     // groups staged in LDS per workgroup
            allow_lds((const void*) cso_compete<16, false>, 128 * 1024);
            hipLaunchKernelGGL((cso_compete<16, false>), dim3((c.ngroup + R - 1) / R, P), dim3(16 * R),
                    (size_t) (R + 2) * c.ld * sizeof(double), stream_, d_, c_);
        }
    });
    if (obj_.needs_host()) host_evaluate(true);
    timed(K_FINISH, [&] {
        hipLaunchKernelGGL(cso_finish_part, dim3(c_.fparts, P), dim3(256), 0, stream_, d_, c_);
        hipLaunchKernelGGL(cso_finish, dim3(P), dim3(64), 0, stream_, d_, c_, 0);
    });
}

void CsoEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    CsoScal s;
    scal_.download(&s, 1, population);
    report_solution(s, X_, ((size_t) population * c_.np + s.ibest) * c_.ld, c_.n, c_.ld, x_out, n_evals,
            converged);
}

int CsoEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const CsoConst &c = c_;
    CsoScal s;
    scal_.download(&s, 1, p);
    const size_t pb = (size_t) p * c.np;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    // per-particle arrays are reported in SLOT order, like the reference's _swarm
    if (k == "x" || k == "v" || k == "pmean") {
        if (k == "pmean" && !c.ring) return 0;
        return o.rows_by_slot(k == "x" ? X_ : k == "v" ? V_ : PM_, occ_, pb, c.np, c.np, c.n, c.ld);
    }
    if (k == "f") return o.vec_by_slot(f_, occ_, pb, c.np, c.np);
    if (k == "home") return o.ints(occ_, pb, c.np);
    // (read-only) the slots as the last generation's shuffle left them, before the sort inside the groups
    if (k == "shuffled") return o.ints(occ2_, pb, c.np);
    if (k == "xbest") return o.vec(X_, (pb + s.ibest) * c.ld, c.n);
    if (k == "mean") return o.vec(mean_, (size_t) p * c.ld, c.n);
    if (k == "meanw") return o.vec(meanw_, (size_t) p * c.ld, c.n);
    if (k == "fbest") return o.one(s.fbest);
    if (k == "np") return o.one(c.np);
    if (k == "fev") return o.one(s.fev);
    if (k == "it") return o.one(s.gen);
    if (k == "stop") return o.one(s.stop);
    if (k == "conv") return o.one(s.conv);
    if (k == "m2") return o.one(s.m2);
    if (k == "phil") return o.one(c.phil);
    if (k == "phih") return o.one(c.phih);
    if (k == "n") return o.one(c.n);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int CsoEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    (void) count;
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_cso_engine(const bbo_params &p)
{
    return new CsoEngine(p);
}

} // namespace bbo
