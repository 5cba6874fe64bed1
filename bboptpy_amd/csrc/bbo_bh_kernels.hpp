// bbo_bh_kernels.hpp -- BasinHopping's hops as gfx950 kernels.
//
//   device function   reference lines (basinhopping.cpp)                                    work per chain
//   bh_collect        :134-137, :162-164 the result of the minimiser, the energy point      n copies, one evaluation
//   bh_decide         :104-107 accept(), :169-189, :50-57 / :72-88 takeStep(), the re-arm   n draws, one exp
//
// bh_hop<Inner> is the kernel around them, one workgroup per chain (one wavefront at n <= 64, 128 threads above), a
// lane per coordinate; the fused launch runs both.  Inner is the view of the minimiser's engine: how its stop,
// its solution() and its evaluation count are read, its own device value function, its own re-arm.  Nothing is
// contracted into a fused multiply-add.
#pragma once

#include "bbo_bh.hpp"
#define BBO_WALK_DEVICE_FUNCTIONS_ONLY     // the minimisers' kernels live in their own translation units
#include "bbo_nm_kernels.hpp"
#include "bbo_rosen_kernels.hpp"

namespace bbo {

#define BH_INF (__builtin_huge_val())

// the uniforms of hop `hop` of sub-stream `sub`: coordinate j's step in [-1, 1), the accept slot in [0, 1)
__host__ __device__ inline double bh_step_uniform(uint64_t seed, uint32_t sub, uint32_t hop, uint32_t j)
{
    const u32x4 w = philox4x32_10(seed, j, 0u, hop, stream_word(STREAM_BH_STEP, sub));
    return u01(w.x, w.y) * 2. - 1.;
}

__host__ __device__ inline double bh_accept_uniform(uint64_t seed, uint32_t sub, uint32_t hop)
{
    const u32x4 w = philox4x32_10(seed, 0u, 0u, hop, stream_word(STREAM_BH_ACCEPT, sub));
    return u01(w.x, w.y);
}

// NelderMead as the minimiser: optimize() returns xmin as nelmin() leaves it (bbo_nm.hip)
struct BhNm {
    using Dev = NmDev;
    using Const = NmConst;
    static __device__ bool stopped(const Dev &d, int p) { return d.scal[p].stop != 0; }
    static __device__ const double *result(const Dev &d, const Const &c, int p) { return d.xmin + (size_t) p * c.ld; }
    static __device__ int fev(const Dev &d, int p) { return d.scal[p].fev; }
    static __device__ int conv(const Dev &d, int p) { return d.scal[p].stop == 1; }
    static __device__ double value(const Dev &d, const Const &c, const double *row, int lane)
    {
        return nm_value(c, row, d.aux, lane);
    }
    static __device__ void rearm(const Dev &d, const Const &c, int p, const double *from, int tid, int nt)
    {
        nm_rearm(d, c, p, from, tid, nt);
    }
};

// Rosenbrock as the minimiser: solution() is x1, which only a converged run has written, or under repair the end
// of the last completed search (bbo_rosen.hip)
struct BhRosen {
    using Dev = RosenDev;
    using Const = RosenConst;
    static __device__ bool stopped(const Dev &d, int p) { return d.scal[p].stop != 0; }
    static __device__ const double *result(const Dev &d, const Const &c, int p)
    {
        const RosenScal *s = d.scal + p;
        if (c.repair && s->stop != 1) return d.x + ((size_t) p * (c.n + 2) + s->i - 1) * c.ld;
        return d.x1 + (size_t) p * c.ld;
    }
    static __device__ int fev(const Dev &d, int p) { return d.scal[p].fev; }
    static __device__ int conv(const Dev &d, int p) { return d.scal[p].stop == 1; }
    static __device__ double value(const Dev &d, const Const &c, const double *row, int lane)
    {
        return rosen_value(c, row, d.aux, lane);
    }
    static __device__ void rearm(const Dev &d, const Const &c, int p, const double *from, int tid, int nt)
    {
        rosen_rearm(d, c, p, from, tid, nt);
    }
};

// slot j < n: the step uniform of coordinate j; slot n: the accept uniform.  From the injected table while it
// covers the hop, from Philox behind it.
__device__ inline double bh_draw(const BhDev &b, const BhConst &c, int p, int hop, int slot)
{
    if (b.inject && hop < c.inject_hops) return b.inject[(size_t) hop * (c.n + 1) + slot];
    const uint32_t sub = (uint32_t) (c.substream + p);
    return slot < c.n ? bh_step_uniform(c.seed, sub, (uint32_t) hop, (uint32_t) slot)
            : bh_accept_uniform(c.seed, sub, (uint32_t) hop);
}

// the value of xsol with the minimiser's own value function, by wavefront 0, into evalue
template<class I>
__device__ inline void bh_evaluate(const BhDev &b, const typename I::Dev &d, const typename I::Const &ic, int p, int ld)
{
    __syncthreads();
    if (threadIdx.x < 64) {
        const double f = I::value(d, ic, b.xsol + (size_t) p * ld, threadIdx.x);
        if (threadIdx.x == 0) b.evalue[p] = f;
    }
    __syncthreads();
}

// takeStep() for hop s.it (:72-79 the adaptive strategy's adjustment first, :52-56 the coordinates and the clamp
// to the box less 5 % on each side), then the re-arm of the minimiser at xtrial
template<class I>
__device__ inline void bh_take_step(const BhDev &b, const BhConst &c, const typename I::Dev &d,
        const typename I::Const &ic, int p, BhScal &s)
{
    const int tid = threadIdx.x, nt = blockDim.x, n = c.n, ld = c.ld, hop = s.it;
    const size_t pv = (size_t) p * ld;
    if (c.adaptive) {
        s.nstep++;
        if (s.nstep % c.interval == 0) {                                // :81-88
            const double acceptp = (1. * s.naccept) / s.nstep;
            if (acceptp > c.accept_rate) s.stepsize /= c.factor;
            else s.stepsize *= c.factor;
        }
    }
    double *start = b.log_start + ((size_t) p * (c.mit + 1) + hop + 1) * ld;
    for (int j = tid; j < ld; j += nt) {
        double xt = 0.;
        if (j < n) {
            const double lo = b.lower[j], up = b.upper[j];
            xt = b.x[pv + j];
            xt += s.stepsize * bh_draw(b, c, p, hop, j) * (up - lo);
            const double margin = 0.05 * (up - lo);
            const double hi = up - margin, lw = lo + margin;
            const double t = hi < xt ? hi : xt;                         // std::min(x[i], upper[i] - margin)
            xt = lw < t ? t : lw;                                       // std::max(lower[i] + margin, .)
        }
        b.xtrial[pv + j] = xt;
        start[j] = xt;
    }
    __syncthreads();
    I::rearm(d, ic, p, b.xtrial + pv, tid, nt);
    s.stage = BH_WAIT_INNER;
}

// A chain that waits for its minimiser, and whose minimiser has stopped: its result by that engine's solution()
// rule into xsol, its evaluation count; under `fused` the energy there, else xsol is left pending.
template<class I>
__device__ inline bool bh_collect(const BhDev &b, const BhConst &c, const typename I::Dev &d,
        const typename I::Const &ic, int p, BhScal &s, bool fused)
{
    if (s.stage != BH_WAIT_INNER || !I::stopped(d, p)) return false;
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t pv = (size_t) p * c.ld;
    const double *res = I::result(d, ic, p);
    for (int j = tid; j < c.ld; j += nt) b.xsol[pv + j] = j < c.n ? res[j] : 0.;
    s.inner_fev = I::fev(d, p);
    s.inner_conv = I::conv(d, p);
    s.stage = BH_WAIT_ENERGY;
    s.pending = 1;
    if (fused) bh_evaluate<I>(b, d, ic, p, c.ld);
    return true;
}

// A chain whose energy point has its value: the first minimisation becomes the incumbent and the best (:135-143),
// a hop goes through the Metropolis test, the strategy's update and the best-so-far rule (:169-182); the log row,
// it++, and below the goal the next step.
template<class I>
__device__ inline bool bh_decide(const BhDev &b, const BhConst &c, const typename I::Dev &d,
        const typename I::Const &ic, int p, BhScal &s)
{
    if (s.stage != BH_WAIT_ENERGY) return false;
    const int tid = threadIdx.x, nt = blockDim.x, ld = c.ld;
    const size_t pv = (size_t) p * ld;
    double e = b.evalue[p];
    if (e != e) e = BH_INF;
    s.pending = 0;
    const int row = s.it + 1;
    bool accept = true, better = true;
    if (s.it < 0) {
        s.energy = e;
        s.bestenergy = e;
    } else {
        const double u = bh_draw(b, c, p, s.it, c.n);                   // drawn on every hop
        const double v = -(e - s.energy) * c.beta;
        const double w = exp(v < 0. ? v : 0.);                          // std::min(0., v): a NaN product accepts
        accept = w >= u;
        if (accept) s.energy = e;
        if (c.adaptive && accept) s.naccept++;
        better = e < s.bestenergy;
        if (better) s.bestenergy = e;
    }
    double *sol = b.log_sol + ((size_t) p * (c.mit + 1) + row) * ld;
    for (int j = tid; j < ld; j += nt) {
        const double xs = b.xsol[pv + j];
        if (accept) b.x[pv + j] = xs;
        if (better) b.xbest[pv + j] = xs;
        sol[j] = xs;
    }
    s.fev += s.inner_fev + 1;
    if (tid == 0) {
        double *lg = b.log + ((size_t) p * (c.mit + 1) + row) * BH_LOG_COLS;
        lg[0] = s.it < 0 ? -1. : (double) s.it;
        lg[1] = e;
        lg[2] = s.inner_conv;
        lg[3] = s.stepsize;
        lg[4] = accept ? 1. : 0.;
        lg[5] = s.bestenergy;
        lg[6] = s.fev;
        b.log_fev[(size_t) p * (c.mit + 1) + row] = s.inner_fev;
    }
    s.rows = row + 1;
    s.it++;
    if (s.it < s.goal) {
        __syncthreads();
        bh_take_step<I>(b, c, d, ic, p, s);
    } else {
        s.stage = BH_IDLE;
        if (tid == 0) atomicAdd(b.done, 1);
    }
    return true;
}

// grid (P), 64 threads (n <= 64) or BH_THREADS
//   mode   BH_FUSED: collect with the evaluation inside, then decide.  BH_COLLECT / BH_EVALUATE / BH_DECIDE: the
//          same in steps, the value of xsol read from `evalue` (a host objective's, or BH_EVALUATE's).
//          BH_BEGIN: the goal becomes min(it + K, mit); an idle chain below it takes its step, one at it counts
//          as finished.
template<class I>
__global__ __launch_bounds__(BH_THREADS) void bh_hop(BhDev b, BhConst c, typename I::Dev d, typename I::Const ic,
        int mode, int K)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    BhScal s = b.scal[p];
    bool touched = false;
    if (mode == BH_BEGIN) {
        const int goal = s.it + K;
        s.goal = goal < c.mit ? goal : c.mit;
        if (s.stage == BH_IDLE) {
            if (s.it < s.goal) bh_take_step<I>(b, c, d, ic, p, s);
            else if (threadIdx.x == 0) atomicAdd(b.done, 1);
        }
        touched = true;
    }
    if (mode == BH_FUSED || mode == BH_COLLECT) touched |= bh_collect<I>(b, c, d, ic, p, s, mode == BH_FUSED);
    if (mode == BH_EVALUATE && s.stage == BH_WAIT_ENERGY && s.pending) bh_evaluate<I>(b, d, ic, p, c.ld);
    if (mode == BH_FUSED || mode == BH_DECIDE) touched |= bh_decide<I>(b, c, d, ic, p, s);
    if (touched && threadIdx.x == 0) b.scal[p] = s;
}

} // namespace bbo
