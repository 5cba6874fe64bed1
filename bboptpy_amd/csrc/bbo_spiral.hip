// bbo_spiral.hip -- host side of the SpiralSearch engine.  Reference behaviour restated on the
// host: SpiralSearch::SpiralSearch / init / optimize / solution (spiral.cpp:46-106, :151-175).
#include "bbo_spiral_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_DRAW = 0, K_ROTATE, K_EVAL, K_BEST, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:spiral_draw", "bbo:spiral_rotate", "bbo:spiral_eval",
        "bbo:spiral_best" };

template<int K>
void launch_rotate_k(int split, dim3 grid, hipStream_t s, const SpiralDev &d, const SpiralConst &c)
{
    const size_t bytes = (size_t) (c.n - split) * 64 * sizeof(double);
    hipLaunchKernelGGL(spiral_rotate<K>, grid, dim3(64), bytes, s, d, c, split);
}
}

SpiralEngine::SpiralEngine(const bbo_params &p) :
        Engine(checked(p))
{
    bbo_spiral_params_default(&sp_);
}

// the part of the constructor's arguments that travels in bbo_params
const bbo_params &SpiralEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_SPIRAL, "SpiralEngine: bad algo");
    BBO_REQUIRE(p.np >= 1 && p.np <= SPIRAL_MAX_NP, "SpiralSearch: np must be in [1, 65536]");
    return p;
}

void SpiralEngine::configure(const bbo_spiral_params &sp)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_spiral_configure after bbo_init");
    const double v[8] = { sp.r, sp.theta, sp.taur, sp.tautheta, sp.rlow, sp.rhigh, sp.thetalow, sp.thetahigh };
    for (double x : v) BBO_REQUIRE(std::isfinite(x), "SpiralSearch: the parameters must be finite");
    sp_ = sp;
}

// the coordinates of a wavefront's tile that LDS holds
int SpiralEngine::lds_coords() const
{
    return SPIRAL_LDS_COORDS;
}

// the coordinates [0, split) of the rotation's tile live in global memory, the rest in LDS
int SpiralEngine::tile_split() const
{
    return (c_.dbg & SPIRAL_DBG_GLOBAL_TILE) ? c_.n : std::max(c_.n - lds_coords(), 0);
}

void SpiralEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    (void) guess;   // SpiralSearch never reads it (spiral.cpp:64-106)
    reject_program(obj, "SpiralSearch");
    BBO_REQUIRE(n >= 1 && n <= SPIRAL_MAX_N, "SpiralSearch: dimension must be in [1, 512]");
    require_finite_box("SpiralSearch draws its points from [lower, upper]: the bounds must be finite", n,
            lower, upper);
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations;
    BBO_REQUIRE((long) P * params_.np <= (1l << 24), "SpiralSearch: populations * np must be <= 2^24");
    const int keep_dbg = c_.dbg, keep_k = c_.kfuse ? c_.kfuse : SPIRAL_DEFAULT_K;
    SpiralConst &c = c_;
    c = SpiralConst {};
    c.n = n;
    c.ld = round_up(n, 2);
    c.np = params_.np;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.dbg = keep_dbg;
    c.kfuse = keep_k;
    c.r = sp_.r; c.theta = sp_.theta; c.taur = sp_.taur; c.tautheta = sp_.tautheta;
    c.rlow = sp_.rlow; c.rhigh = sp_.rhigh; c.thetalow = sp_.thetalow; c.thetahigh = sp_.thetahigh;
    c.seed = params_.seed;

    const size_t rows = (size_t) P * c.np;
    X_.alloc(rows * c.ld);
    f_.alloc(rows);
    r_.alloc(rows);
    theta_.alloc(rows);
    cs_.alloc(rows);
    sn_.alloc(rows);
    xbest_.alloc((size_t) P * c.ld);
    tables_.clear();
    tile_.alloc(0);
    tile_split_ = 0;
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    std::vector<SpiralScal> sc(P);
    for (auto &s : sc) {
        std::memset(&s, 0, sizeof(s));
        s.fev = c.np;           // the initial points are evaluated (spiral.cpp:95)
        s.fbest = std::numeric_limits<double>::infinity();
    }
    scal_.upload(sc.data(), P);

    SpiralDev &d = d_;
    d = SpiralDev {};
    d.X = X_.p; d.f = f_.p; d.r = r_.p; d.theta = theta_.p; d.cs = cs_.p; d.sn = sn_.p;
    d.xbest = xbest_.p; d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.scal = scal_.p;
    inited_ = true;

    hipLaunchKernelGGL(spiral_init, dim3((c.np + 3) / 4, P), dim3(256), 0, stream_, d_, c_);
    BBO_HIP(hipGetLastError());
    launch_eval(0, P);
    launch_best(0, P, 0);
    BBO_HIP(hipStreamSynchronize(stream_));
}

void SpiralEngine::launch_draw()
{
    const long total = (long) c_.npop * c_.np;
    timed(K_DRAW, [&] {
        hipLaunchKernelGGL(spiral_draw, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, stream_, d_, c_);
    });
}

void SpiralEngine::launch_rotate()
{
    const long total = (long) c_.npop * c_.np;
    const dim3 grid((unsigned) ((total + 63) / 64));
    const int split = tile_split();
    if (split > tile_split_) {
        tile_.alloc((size_t) grid.x * split * 64);
        BBO_HIP(hipDeviceSynchronize());    // (the allocation's fill runs on another stream)
        tile_split_ = split;
    }
    d_.tile = tile_.p;
    timed(K_ROTATE, [&] {
        switch (c_.kfuse) {
        case 1: launch_rotate_k<1>(split, grid, stream_, d_, c_); break;
        case 2: launch_rotate_k<2>(split, grid, stream_, d_, c_); break;
        case 4: launch_rotate_k<4>(split, grid, stream_, d_, c_); break;
        default: launch_rotate_k<8>(split, grid, stream_, d_, c_); break;
        }
    });
}

void SpiralEngine::launch_eval(int p0, int pcount)
{
    if (obj_.needs_host()) {
        // the rows of the populations p0 .. p0 + pcount - 1 in row order, like the reference's loop
        host_evaluate_range(X_, f_, p0, pcount, c_.np, 0, c_.np, c_.n, c_.ld, c_.honor_stop != 0);
        return;
    }
    timed(K_EVAL, [&] {
        hipLaunchKernelGGL(spiral_eval, dim3((c_.np + 3) / 4, pcount), dim3(256), 0, stream_, d_, c_, p0);
    });
}

void SpiralEngine::launch_best(int p0, int pcount, int counters)
{
    timed(K_BEST, [&] { hipLaunchKernelGGL(spiral_best, dim3(pcount), dim3(256), 0, stream_, d_, c_, p0, counters); });
}

void SpiralEngine::generation(bool honor_stop)
{
    c_.honor_stop = honor_stop ? 1 : 0;
    launch_draw();
    launch_rotate();
    launch_eval(0, c_.npop);
    launch_best(0, c_.npop, 1);
}

// the four parts of iterate(), one at a time
void SpiralEngine::phase(int which)
{
    run_phase("bbo_spiral_phase", which, 4, "bbo_spiral_phase: 0 draw, 1 rotate, 2 evaluate, 3 best", [&] {
        c_.honor_stop = 0;
        if (which == 0) launch_draw();
        else if (which == 1) launch_rotate();
        else if (which == 2) launch_eval(0, c_.npop);
        else launch_best(0, c_.npop, 1);
    });
}

void SpiralEngine::inject_uniforms(const double *u, int count)
{
    enter("bbo_spiral_inject_uniforms");
    BBO_HIP(hipStreamSynchronize(stream_));
    if (!u) {
        d_.inject = nullptr;
        return;
    }
    const size_t want = (size_t) c_.npop * c_.np * 4;
    BBO_REQUIRE(count >= 0 && (size_t) count == want, "bbo_spiral_inject_uniforms: populations * np * 4 values");
    for (size_t q = 0; q < want; q++)
        BBO_REQUIRE(u[q] >= 0. && u[q] < 1., "bbo_spiral_inject_uniforms: uniforms lie in [0, 1)");
    d_.inject = tables_.load(u, want);
}

void SpiralEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    SpiralScal s;
    scal_.download(&s, 1, population);
    report_solution(s, xbest_, (size_t) population * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

int SpiralEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const SpiralConst &c = c_;
    SpiralScal s;
    scal_.download(&s, 1, p);
    const size_t pb = (size_t) p * c.np;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    if (k == "x") return o.rows(X_, pb, c.np, c.n, c.ld);
    if (k == "f") return o.vec(f_, pb, c.np);
    if (k == "r") return o.vec(r_, pb, c.np);
    if (k == "theta") return o.vec(theta_, pb, c.np);
    if (k == "cos") return o.vec(cs_, pb, c.np);
    if (k == "sin") return o.vec(sn_, pb, c.np);
    if (k == "xbest") return o.vec(xbest_, (size_t) p * c.ld, c.n);
    if (k == "draws") {
        require_record(c.record, k);
        return o.vec(tables_.draws, pb * 4, c.np * 4);
    }
    if (k == "fbest") return o.one(s.fbest);
    if (k == "ibest") return o.one(s.ibest);
    if (k == "fev") return o.one(s.fev);
    if (k == "it") return o.one(s.it);
    if (k == "flag" || k == "stop") return o.one(s.stop);
    if (k == "record_draws") return o.one(c.record);
    if (k == "dbg") return o.one(c.dbg);
    if (k == "rot_k") return o.one(c.kfuse);
    if (k == "rot_split") return o.one(tile_split());
    if (k == "rot_lds_coords") return o.one(lds_coords());
    if (k == "np") return o.one(c.np);
    if (k == "n") return o.one(c.n);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int SpiralEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    const SpiralConst &c = c_;
    const size_t pb = (size_t) p * c.np;
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "record_draws") {      // (the whole handle: every population)
        BBO_REQUIRE(count == 1, "record_draws: one value");
        c_.record = in[0] != 0. ? 1 : 0;
        d_.draws = tables_.record(c_.record != 0, (size_t) c.npop * c.np * 4);
        return 1;
    }
    if (k == "dbg") {
        BBO_REQUIRE(count == 1 && (in[0] == 0. || in[0] == 1.), "dbg: 0, or 1 (the whole tile of the rotation in global memory)");
        c_.dbg = (int) in[0];
        return 1;
    }
    if (k == "rot_k") {
        BBO_REQUIRE(count == 1 && (in[0] == 1. || in[0] == 2. || in[0] == 4. || in[0] == 8.), "rot_k: 1, 2, 4 or 8");
        c_.kfuse = (int) in[0];
        return 1;
    }
    if (k == "x") {             // f, ibest and xbest follow; fev does not move
        BBO_REQUIRE(count == c.np * c.n, "x: np * n values");
        upload_rows(X_, pb, c.np, c.n, c.ld, in);
        c_.honor_stop = 0;
        launch_eval(p, 1);
        launch_best(p, 1, 0);
        BBO_HIP(hipStreamSynchronize(stream_));
        return count;
    }
    if (k == "r") {
        BBO_REQUIRE(count == c.np, "r: np values");
        r_.upload(in, c.np, pb);
        return count;
    }
    if (k == "theta") {         // cos and sin follow
        BBO_REQUIRE(count == c.np, "theta: np values");
        std::vector<double> cs(c.np), sn(c.np);
        for (int i = 0; i < c.np; i++) {
            cs[i] = std::cos(in[i]);
            sn[i] = std::sin(in[i]);
        }
        theta_.upload(in, c.np, pb);
        cs_.upload(cs.data(), c.np, pb);
        sn_.upload(sn.data(), c.np, pb);
        return count;
    }
    if (k == "fev") {           // (the budget test looks at it after the next generation)
        BBO_REQUIRE(count == 1 && in[0] >= 0. && in[0] == std::floor(in[0]) && in[0] < 2147483647.,
                "fev: one non-negative integer");
        SpiralScal s;
        scal_.download(&s, 1, p);
        s.fev = (int) in[0];
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_spiral_engine(const bbo_params &p)
{
    return new SpiralEngine(p);
}

} // namespace bbo
