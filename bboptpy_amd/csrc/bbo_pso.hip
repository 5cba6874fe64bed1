// bbo_pso.hip -- host side of the APSO engine.
// Reference behaviour restated on the host: APSOSearch::init/optimize/solution
// (apso.cpp:48-127).
#include "bbo_pso_kernels.hpp"

#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_CENTER = 0, K_ESE, K_CTRL, K_UPDATE, K_FINISH, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:pso_center", "bbo:pso_ese", "bbo:pso_control", "bbo:pso_update", "bbo:pso_finish" };   // roctx ranges, bench.py's slot names
}

PsoEngine::PsoEngine(const bbo_params &p) :
        Engine(checked(p))
{
}

// the algorithm's own parameter checks, ahead of the base's (populations, device)
const bbo_params &PsoEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_APSO, "PsoEngine: bad algo");
    BBO_REQUIRE(p.np >= 2, "APSO needs at least 2 particles");
    return p;
}

void PsoEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    (void) guess;   // APSO never reads it (apso.cpp:48-103)
    reject_program(obj, "APSO");
    BBO_REQUIRE(n >= 1 && n <= 2048, "APSO: dimension must be in [1, 2048]");
    require_finite_box("APSO draws its swarm from [lower, upper]: the bounds must be finite", n,
            lower, upper);
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations;
    PsoConst &c = c_;
    c = PsoConst {};
    c.n = n;
    c.ld = round_up(n, 2);
    c.np = params_.np;
    c.ldc = round_up(n, 16);
    c.npad = round_up(params_.np, 128);
    c.correct = params_.correct ? 1 : 0;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.tol = params_.tol;
    c.seed = params_.seed;
    parts_ = std::max(1, std::min(256, c.np / 64));
    {   // up to 16 refreshes of the swarm's best per generation, chunks of at least 64 particles
        // (multiples of 16: whole workgroups); a swarm of up to 64 moves in one piece
        // (beyond 32768 particles eight: a launch over fewer than ~8000 particles is one round of
        // workgroups and leaves HBM half idle -- C4's update ran at 0.37 of the roof in 16 chunks)
        const int nchunks = c.np > 32768 ? 8 : std::min(16, (c.np + 63) / 64);
        chunk_ = ((c.np + nchunks - 1) / nchunks + 15) / 16 * 16;
        if (nchunks <= 1) chunk_ = c.np;
    }

    const size_t rows = (size_t) P * c.np, ld = c.ld;
    X_.alloc(rows * ld);
    V_.alloc(rows * ld);
    XB_.alloc(rows * ld);
    f_.alloc(rows);
    fb_.alloc(rows);
    xbest_.alloc(P * ld);
    ws_.alloc(rows);
    mean_.alloc(P * ld);
    nrm_.alloc(rows);
    Xc_.alloc((size_t) P * c.npad * c.ldc);     // zeroed: the padding is never written
    pvec_.alloc(P * ld);
    radius_.alloc(rows);
    colpart_.alloc((size_t) P * parts_ * ld);
    colpart2_.alloc((size_t) P * ((c.np + 127) / 128) * c.np);
    rowpart2_.alloc(rows);
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    std::vector<PsoScal> sc(P);
    for (auto &s : sc) {
        std::memset(&s, 0, sizeof(s));
        s.w = 0.9;
        s.c1 = s.c2 = 2.;
        s.fbest = std::numeric_limits<double>::infinity();
        s.maxit = (int) std::round(params_.mfev / (1. + c.np));   // apso.cpp:68
        s.fev = c.np;
    }
    scal_.upload(sc.data(), P);

    PsoDev &d = d_;
    d = PsoDev {};
    d.X = X_.p; d.V = V_.p; d.XB = XB_.p; d.f = f_.p; d.fb = fb_.p; d.xbest = xbest_.p;
    d.ws = ws_.p; d.mean = mean_.p; d.nrm = nrm_.p; d.Xc = Xc_.p; d.pvec = pvec_.p; d.radius = radius_.p;
    d.colpart = colpart_.p; d.colpart2 = colpart2_.p; d.rowpart2 = rowpart2_.p; d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p;
    d.scal = scal_.p;
    c.honor_stop = 0;
    inited_ = true;

    dim3 g16((c.np + 15) / 16, P);
    const int R = rows_per_wg16(c.ld);
    hipLaunchKernelGGL(pso_init, dim3((c.np + R - 1) / R, P), dim3(16 * R),
            (size_t) R * c.ld * sizeof(double), stream_, d_, c_);
    BBO_HIP(hipGetLastError());
    if (obj_.needs_host()) {
        host_evaluate_range(X_, f_, 0, P, c.np, 0, c.np, c.n, c.ld);
        hipLaunchKernelGGL(pso_copy_fb, dim3((c.np + 255) / 256, P), dim3(256), 0, stream_, d_,
                c_);
        BBO_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(pso_gbest_init, dim3(P), dim3(256), 0, stream_, d_, c_);
    BBO_HIP(hipGetLastError());
    BBO_HIP(hipStreamSynchronize(stream_));
}

void PsoEngine::host_evaluate_elite()
{
    const PsoConst &c = c_;
    BBO_HIP(hipStreamSynchronize(stream_));
    std::vector<PsoScal> sc(c.npop);
    scal_.download(sc.data(), c.npop);
    std::vector<double> pv(c.ld);
    bool touched = false;
    for (int p = 0; p < c.npop; p++) {
        if ((c.honor_stop && sc[p].stop) || !sc[p].need_elite) continue;
        pvec_.download(pv.data(), c.ld, (size_t) p * c.ld);
        double f = 0.;
        obj_.eval_host(pv.data(), 1, c.n, c.ld, &f);
        nan_to_inf(&f, 1);
        sc[p].nu = f;
        touched = true;
    }
    if (touched) scal_.upload(sc.data(), c.npop);
}

void PsoEngine::generation(bool honor_stop)
{
    PsoConst &c = c_;
    c.honor_stop = honor_stop ? 1 : 0;
    const int P = c.npop;
    dim3 g16((c.np + 15) / 16, P);
    const int R = rows_per_wg16(c.ld);     // rows staged in LDS per workgroup
    const size_t ldsR = (size_t) R * c.ld * sizeof(double);
    timed(K_CENTER, [&] {
        hipLaunchKernelGGL(pso_center, dim3(parts_, P), dim3(256), 0, stream_, d_, c_, parts_);
        hipLaunchKernelGGL(pso_mean, dim3(P), dim3(256), 0, stream_, d_, c_, parts_);
        hipLaunchKernelGGL(pso_nrm, g16, dim3(256), 0, stream_, d_, c_);
    });
    timed(K_ESE, [&] {
        const size_t lds = (size_t) ESE2_LDS_DOUBLES * sizeof(double);
        allow_lds((const void*) pso_ese_sym, (int) lds);
        hipLaunchKernelGGL(pso_ese_sym, dim3((c.np + 127) / 128, P), dim3(256), lds, stream_, d_,
                c_);
        hipLaunchKernelGGL(pso_ese_finish, dim3((c.np + 255) / 256, P), dim3(256), 0, stream_, d_,
                c_);
    });
    timer_.begin(stream_, K_CTRL);      // (the host's evaluation of the elite lies between its two launches)
    hipLaunchKernelGGL(pso_control_a, dim3(P), dim3(256), 0, stream_, d_, c_);
    BBO_HIP(hipGetLastError());
    if (obj_.needs_host()) host_evaluate_elite();
    hipLaunchKernelGGL(pso_control_b, dim3(P), dim3(256), 0, stream_, d_, c_);
    timer_.end(stream_);
    BBO_HIP(hipGetLastError());
    // the swarm moves in chunks of chunk_ particles, the best refreshed between them: what the
    // reference's in-loop refresh (apso.cpp:194-197) buys at large np (one chunk = the generation-
    // synchronous form of rounds 1-4: every particle sees the best of the generation start)
    const int step = chunk_ > 0 && chunk_ < c.np ? chunk_ : c.np;
    // (the timer slots: pso_update brackets each update launch, pso_finish the refreshes of the best
    // and the closing kernel)
    for (int i0 = 0; i0 < c.np; i0 += step) {
        const int i1 = std::min(c.np, i0 + step);
        timed(K_UPDATE, [&] {
            hipLaunchKernelGGL(pso_update, dim3((i1 - i0 + R - 1) / R, P), dim3(16 * R), ldsR, stream_, d_,
                    c_, i0, i1);
        });
        if (obj_.needs_host()) {
            host_evaluate_range(X_, f_, 0, P, c.np, i0, i1, c.n, c.ld, c.honor_stop != 0);   // (this chunk's particles)
            hipLaunchKernelGGL(pso_pbest, dim3((i1 - i0 + 15) / 16, P), dim3(256), 0, stream_, d_, c_, i0,
                    i1);
        }
        if (i1 < c.np)
            timed(K_FINISH, [&] { hipLaunchKernelGGL(pso_gbest, dim3(P), dim3(256), 0, stream_, d_, c_, i0, i1); });
    }
    BBO_HIP(hipGetLastError());     // (pso_pbest's)
    timed(K_FINISH, [&] { hipLaunchKernelGGL(pso_finish, dim3(P), dim3(256), 0, stream_, d_, c_); });
}

void PsoEngine::inspect(const std::vector<PsoScal> &sc)
{
    for (const auto &s : sc)
        if (s.bad_rule)
            throw Error(BBO_ERR_ARG,
                    "Error [PSO]: Invalid rule base. Please report this issue on Github.");
}

void PsoEngine::after_chunk(bool in_run)
{
    if (in_run) return;      // (run() sees the scalars at its next poll)
    std::vector<PsoScal> sc(c_.npop);
    scal_.download(sc.data(), c_.npop);
    inspect(sc);
}

void PsoEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    PsoScal s;
    scal_.download(&s, 1, population);
    report_solution(s, xbest_, (size_t) population * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
    if (s.it == 0)
        *converged = radius_spread_converged(radius_, (size_t) population * c_.np, c_.np, c_.tol);
}

int PsoEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const PsoConst &c = c_;
    PsoScal s;
    scal_.download(&s, 1, p);
    const StateOut o { out, cap };
    const size_t pb = (size_t) p * c.np;
    if (k == "profile") return profile_report(out, cap);
    if (k == "x") return o.rows(X_, pb, c.np, c.n, c.ld);
    if (k == "v") return o.rows(V_, pb, c.np, c.n, c.ld);
    if (k == "xb") return o.rows(XB_, pb, c.np, c.n, c.ld);
    if (k == "f") return o.vec(f_, pb, c.np);
    if (k == "fb") return o.vec(fb_, pb, c.np);
    if (k == "ws") return o.vec(ws_, pb, c.np);
    if (k == "xbest") return o.vec(xbest_, (size_t) p * c.ld, c.n);
    if (k == "fbest") return o.one(s.fbest);
    if (k == "w") return o.one(s.w);
    if (k == "c1") return o.one(s.c1);
    if (k == "c2") return o.one(s.c2);
    if (k == "state") return o.one(s.state);
    if (k == "it") return o.one(s.it);
    if (k == "maxit") return o.one(s.maxit);
    if (k == "fev") return o.one(s.fev);
    if (k == "np") return o.one(c.np);
    if (k == "chunk") return o.one(chunk_);      // particles between two refreshes of the swarm's best
    if (k == "evof") return o.one(s.evof);
    if (k == "stop") return o.one(s.stop);
    if (k == "conv") return o.one(s.conv);
    if (k == "m2") return o.one(s.m2);
    if (k == "n") return o.one(c.n);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int PsoEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    const PsoConst &c = c_;
    if (k == "chunk") {        // 0 or >= np: the whole swarm sees the best of the generation start
        BBO_REQUIRE(count == 1, "set: wrong element count");
        BBO_REQUIRE(std::isfinite(in[0]) && in[0] >= 0., "set: chunk must be finite and >= 0");
        chunk_ = in[0] < 1. || in[0] >= (double) c.np ? c.np : (int) in[0];
        return 1;
    }
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "x" || k == "v" || k == "xb") {
        BBO_REQUIRE(count == c.np * c.n, "set: wrong element count");
        upload_rows(k == "x" ? X_ : k == "v" ? V_ : XB_, (size_t) p * c.np, c.np, c.n, c.ld, in);
        return count;
    }
    if (k == "f" || k == "fb") {
        BBO_REQUIRE(count == c.np, "set: wrong element count");
        (k == "f" ? f_ : fb_).upload(in, c.np, (size_t) p * c.np);
        return count;
    }
    if (k == "xbest") {
        BBO_REQUIRE(count == c.n, "set: wrong element count");
        xbest_.upload(in, c.n, (size_t) p * c.ld);
        return count;
    }
    BBO_REQUIRE(count == 1, "set: wrong element count");
    PsoScal s;
    scal_.download(&s, 1, p);
    if (k == "fbest") s.fbest = in[0];
    else if (k == "w") s.w = in[0];
    else if (k == "c1") s.c1 = in[0];
    else if (k == "c2") s.c2 = in[0];
    else if (k == "state") s.state = (int) in[0];
    else if (k == "it") s.it = (int) in[0];
    else if (k == "fev") s.fev = (int) in[0];
    else if (k == "stop") s.stop = (int) in[0];
    else throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
    scal_.upload(&s, 1, p);
    return 1;
}

Optimizer* make_pso_engine(const bbo_params &p)
{
    return new PsoEngine(p);
}

} // namespace bbo
