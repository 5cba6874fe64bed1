// bbo_spiral_kernels.hpp -- one SpiralSearch generation as gfx950 kernels.
//
//   kernel          reference lines (spiral.cpp)                          work per point
//   spiral_init     :84-87 uniform points, :100-105 r, theta              8n written
//   spiral_draw     :111-118 the coins and the new r / theta,             two Philox calls
//                   :124-125 cos, sin (kept as state)
//   spiral_rotate   :126-134, :177-190: rotate_n of x_i - xbest and       n (n - 1) / 2 rotations of
//                   x_i = r_i (R d) + xbest                               6 fp64 operations each
//   spiral_eval     :141 the objective                                    8n read
//   spiral_best     :138-148 the first strict minimum, xbest, fev, it;    8
//                   :163 the budget
#pragma once

#include "bbo_spiral.hpp"
#include "bbo_objectives.hpp"
#include "bbo_rng.hpp"
#include "bbo_wave.hpp"

namespace bbo {

#define SPIRAL_INF (__builtin_huge_val())

// Random::get(a, b) of the reference on doubles (random.hpp:329-337) over the raw uniform u
__device__ inline double spiral_between(double u, double a, double b)
{
#pragma clang fp contract(off)
    const double lo = a < b ? a : b, hi = a < b ? b : a;
    return u * (hi - lo) + lo;
}

// :84-87, :100-105: a wavefront per point.  grid (ceil(np / 4), P), 256 threads
__global__ __launch_bounds__(256) void spiral_init(SpiralDev d, SpiralConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave, n = c.n;
    if (i >= c.np) return;
    const size_t row = (size_t) p * c.np + i;
    double *x = d.X + row * c.ld;
    for (int j = lane; j < n; j += 64) {
        const u32x4 w = philox4x32_10(c.seed, (uint32_t) i, (uint32_t) j, 0,
                stream_word(STREAM_INIT, (uint32_t) p));
        x[j] = u01(w.x, w.y) * (d.upper[j] - d.lower[j]) + d.lower[j];
    }
    if (lane == 0) {
        d.r[row] = c.r;
        d.theta[row] = c.theta;
        d.cs[row] = cos(c.theta);
        d.sn[row] = sin(c.theta);
    }
}

// :111-118.  A thread per point; the four uniforms of a point come from the two counter positions
// (point, 0 / 1, generation) of the population's sub-stream whichever coins fire: (coin of r, value
// of r), (coin of theta, value of theta).  cos and sin are recomputed for the angles that changed.
// grid (ceil(P np / 256)), 256 threads
__global__ __launch_bounds__(256) void spiral_draw(SpiralDev d, SpiralConst c)
{
#pragma clang fp contract(off)
    const long total = (long) c.npop * c.np;
    const long g = (long) blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int p = (int) (g / c.np), i = (int) (g - (long) p * c.np);
    const SpiralScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    double u[4];
    if (d.inject) {
#pragma unroll
        for (int q = 0; q < 4; q++) u[q] = d.inject[g * 4 + q];
    } else {
        const uint32_t sw = stream_word(STREAM_SPIRAL, (uint32_t) p);
        const u32x4 w0 = philox4x32_10(c.seed, (uint32_t) i, 0, (uint32_t) sc->it, sw);
        const u32x4 w1 = philox4x32_10(c.seed, (uint32_t) i, 1, (uint32_t) sc->it, sw);
        u[0] = u01(w0.x, w0.y);
        u[1] = u01(w0.z, w0.w);
        u[2] = u01(w1.x, w1.y);
        u[3] = u01(w1.z, w1.w);
    }
    if (u[0] < c.taur) d.r[g] = spiral_between(u[1], c.rlow, c.rhigh);
    if (u[2] < c.tautheta) {
        const double th = spiral_between(u[3], c.thetalow, c.thetahigh);
        d.theta[g] = th;
        d.cs[g] = cos(th);
        d.sn[g] = sin(th);
    }
    if (d.draws) {
#pragma unroll
        for (int q = 0; q < 4; q++) d.draws[g * 4 + q] = u[q];
    }
}

// rotate(), :177-182: the two products, then -; the two products, then +
__device__ inline void spiral_rot(double cs, double sn, double &xa, double &xb)
{
#pragma clang fp contract(off)
    const double na = cs * xa - sn * xb;
    const double nb = sn * xa + cs * xb;
    xa = na;
    xb = nb;
}

// The hot path.  One lane per point: the grid spans the P np points of the handle, so the points
// of several populations share a wavefront.  The lane keeps d = x_i - xbest coordinate-major, 64
// lanes side by side: the coordinates [split, n) in LDS at lt[(j - split) * 64 + lane] (a
// wavefront's accesses fall on distinct banks), the coordinates [0, split) in a global tile of the
// same shape (coalesced).  split = max(n - SPIRAL_LDS_COORDS, 0): coordinate j is visited by the
// stages a < j only, so the low coordinates, which leave the walk first, are the ones that can
// afford the longer way, and 40 KiB of LDS per wavefront leave room for four on a CU.  The lane
// walks rotate_n's sequence (:184-190), stage a = 0 .. n - 2 against b = a + 1 .. n - 1, in the
// reference's order.  K consecutive stages are fused: the K x K triangle among the pivots
// a .. a + K - 1 is settled in registers, then every streamed d_b takes its K rotations between one
// read and one write.  Every element sees the same operations in the same order as with K = 1 and
// wherever it is kept: the same bits, 1 / K of the tile traffic.  No lane reads another lane's data.
// grid (ceil(P np / 64)), 64 threads, LDS 64 (n - split) doubles
template<int K>
__global__ __launch_bounds__(64) void spiral_rotate(SpiralDev d, SpiralConst c, int split)
{
#pragma clang fp contract(off)
    extern __shared__ double spiral_lds[];
    const int lane = threadIdx.x, n = c.n;
    const long total = (long) c.npop * c.np;
    const long g = (long) blockIdx.x * 64 + lane;
    if (g >= total) return;
    const int p = (int) (g / c.np);
    if (pop_frozen(c, d.scal + p)) return;
    double *lt = spiral_lds + lane;
    double *gt = d.tile + (size_t) blockIdx.x * split * 64 + lane;     // (never touched when split == 0)
    double *x = d.X + (size_t) g * c.ld;
    const double *xb = d.xbest + (size_t) p * c.ld;
    const double cs = d.cs[g], sn = d.sn[g], r = d.r[g];
    const auto load = [&](int j) { return j < split ? gt[(size_t) j * 64] : lt[(j - split) * 64]; };
    const auto store = [&](int j, double v) {
        if (j < split) gt[(size_t) j * 64] = v;
        else lt[(j - split) * 64] = v;
    };
    for (int j = 0; j < n; j++) store(j, x[j] - xb[j]);
    int a = 0;
    for (; a + K <= n - 1; a += K) {
        double pv[K];
#pragma unroll
        for (int k = 0; k < K; k++) pv[k] = load(a + k);
#pragma unroll
        for (int k = 0; k < K; k++)
#pragma unroll
            for (int m = k + 1; m < K; m++) spiral_rot(cs, sn, pv[k], pv[m]);
        int b = a + K;
#pragma unroll 2
        for (; b < split; b++) {
            double v = gt[(size_t) b * 64];
#pragma unroll
            for (int k = 0; k < K; k++) spiral_rot(cs, sn, pv[k], v);
            gt[(size_t) b * 64] = v;
        }
#pragma unroll 2
        for (; b < n; b++) {
            double v = lt[(b - split) * 64];
#pragma unroll
            for (int k = 0; k < K; k++) spiral_rot(cs, sn, pv[k], v);
            lt[(b - split) * 64] = v;
        }
#pragma unroll
        for (int k = 0; k < K; k++) store(a + k, pv[k]);
    }
    // the stages a fused step no longer fits, one at a time
    for (; a < n - 1; a++) {
        double pa = load(a);
        for (int b = a + 1; b < n; b++) {
            double v = load(b);
            spiral_rot(cs, sn, pa, v);
            store(b, v);
        }
        store(a, pa);
    }
    for (int j = 0; j < n; j++) x[j] = r * load(j) + xb[j];
}

// :141: a wavefront per point of the populations p0 .. p0 + gridDim.y - 1.
// grid (ceil(np / 4), populations), 256 threads
__global__ __launch_bounds__(256) void spiral_eval(SpiralDev d, SpiralConst c, int p0)
{
#pragma clang fp contract(off)
    const int p = p0 + blockIdx.y;
    if (pop_frozen(c, d.scal + p)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    if (i >= c.np) return;
    const size_t row = (size_t) p * c.np + i;
    double f = eval_row_group<64>(c.obj, c.n, d.X + row * c.ld, d.aux, lane);
    if (f != f) f = SPIRAL_INF;
    if (lane == 0) d.f[row] = f;
}

// :138-148: the first strict minimum of this generation's values in row order (ties to the lower
// row), its row to xbest; with `counters` fev += np, it++ and the budget of :163.
// grid (populations), 256 threads
__global__ __launch_bounds__(256) void spiral_best(SpiralDev d, SpiralConst c, int p0, int counters)
{
    const int p = p0 + blockIdx.x;
    SpiralScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    __shared__ double sval[4];
    __shared__ int sidx[4];
    const int tid = threadIdx.x, np = c.np;
    const size_t pb = (size_t) p * np;
    double fmin = SPIRAL_INF;
    int rmin = 0x7fffffff;
    for (int i = tid; i < np; i += 256) {
        const double fv = d.f[pb + i];
        if (fv < fmin || (fv == fmin && i < rmin)) {
            fmin = fv;
            rmin = i;
        }
    }
    block_arg<1>(fmin, rmin, sval, sidx);
    rmin = min(rmin, np - 1);
    for (int j = tid; j < c.ld; j += 256)
        d.xbest[(size_t) p * c.ld + j] = d.X[(pb + rmin) * c.ld + j];
    if (tid != 0) return;
    sc->fbest = fmin;
    sc->ibest = rmin;
    sc->conv = 0;
    if (!counters) return;
    sc->fev += np;
    sc->it++;
    if (sc->fev >= c.mfev) sc->stop = 2;
}

} // namespace bbo
