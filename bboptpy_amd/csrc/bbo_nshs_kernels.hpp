// bbo_nshs_kernels.hpp -- NSHS as gfx950 kernels.
//
//   kernel          reference lines (nshs.cpp)                            work per population
//   nshs_init       :60-67 uniform rows and their values, :70-74 fstd,    hms rows
//                   best (and the worst, which :157 finds later)
//   nshs_generate   :112-147 the candidate                                n coordinates
//   nshs_eval       :150 its value                                        one row
//   nshs_replace    :157-169 replacement, fstd, best; :96, :151 counters  hms values
//   nshs_steps      K times the three above in one launch                 K iterations
#pragma once

#include "bbo_nshs.hpp"
#include "bbo_objectives.hpp"
#include "bbo_rng.hpp"
#include "bbo_wave.hpp"

namespace bbo {

#define NSHS_INF (__builtin_huge_val())

enum NshsInitMode { NSHS_INIT_DRAW = 1, NSHS_INIT_EVAL = 2 };

// Random::get(a, b) of the reference on doubles (random.hpp:329-337) over the raw uniform u
__device__ inline double nshs_between(double u, double a, double b)
{
#pragma clang fp contract(off)
    const double lo = a < b ? a : b, hi = a < b ? b : a;
    return u * (hi - lo) + lo;
}

// The four raw uniforms of coordinate i in iteration `it` of population p: the coin and the row
// from counter (i, 0, it), the fresh value and the adjustment from (i, 1, it), whichever of them
// the iteration uses.  Nothing else enters the key: not K, not the route, not P.
__device__ inline void nshs_uniforms(const NshsDev &d, const NshsConst &c, int p, int i, int it,
        double &u0, double &u1, double &u2, double &u3)
{
    const size_t q = ((size_t) p * c.n + i) * 4;
    if (d.inject) {
        u0 = d.inject[q];
        u1 = d.inject[q + 1];
        u2 = d.inject[q + 2];
        u3 = d.inject[q + 3];
    } else {
        const uint32_t sw = stream_word(STREAM_NSHS, (uint32_t) p);
        const u32x4 w0 = philox4x32_10(c.seed, (uint32_t) i, 0, (uint32_t) it, sw);
        const u32x4 w1 = philox4x32_10(c.seed, (uint32_t) i, 1, (uint32_t) it, sw);
        u0 = u01(w0.x, w0.y);
        u1 = u01(w0.z, w0.w);
        u2 = u01(w1.x, w1.y);
        u3 = u01(w1.z, w1.w);
    }
    if (d.draws) {
        d.draws[q] = u0;
        d.draws[q + 1] = u1;
        d.draws[q + 2] = u2;
        d.draws[q + 3] = u3;
    }
}

// :118-146 for coordinate i.  hm: the rows of the memory, [hms][ld], in LDS or global memory.  One
// IEEE operation per operation of the reference, in its order; std::min / std::max as libstdc++
// writes them.  Only a lane whose coin failed in the narrow branch scans its column.
__device__ inline double nshs_coordinate(const NshsConst &c, const double *hm, double lo, double up,
        int i, int wide, int it, double u0, double u1, double u2, double u3)
{
#pragma clang fp contract(off)
    double x;
    if (u0 < c.hmcr) {
        const int j = min((int) (u1 * (double) c.hms), c.hms - 1);
        x = hm[(size_t) j * c.ld + i];
    } else if (wide) {
        x = nshs_between(u2, lo, up);
    } else {
        double mn = up, mx = lo;
        for (int j = 0; j < c.hms; j++) {
            const double v = hm[(size_t) j * c.ld + i];
            mn = v < mn ? v : mn;
            mx = mx < v ? v : mx;
        }
        x = nshs_between(u2, mn, mx);
    }
    if (wide) {
        const double bw = ((up - lo) / c.tunerange) * (1.0 - (1. * it) / c.mit);
        x += nshs_between(u3, -bw, bw);
    } else {
        x += nshs_between(u3, -c.fstdmin, c.fstdmin);
    }
    x = up < x ? up : x;
    x = x < lo ? lo : x;
    return x;
}

// The statistics of the memory's values, by ONE wavefront: the first minimum and the first maximum
// (ties to the lowest row) and fstd in its device form.  The shape of the sums is part of the
// specification (tests/nshs_model.py, tree_sum): lane l adds the rows l, l + 64, l + 128, ... in
// this order starting from 0, then the 64 partial sums meet in the xor butterfly of group_sum<64>
// (offsets 32, 16, .., 1).  mean = sum / hms; m2 = the same sum over (f - mean)^2;
// fstd = sqrt(m2 / hms).  An inf among the values gives mean = inf, inf - inf = NaN and fstd = NaN:
// `fstd > fstdmin` is false, the narrow branch.  Every lane returns the same values.
__device__ inline void nshs_select(const double *f, int hms, int lane, double fstdmin, NshsScal &s)
{
#pragma clang fp contract(off)
    double fmin = NSHS_INF, fmax = -NSHS_INF, sum = 0.;
    int imin = 0x7fffffff, imax = 0x7fffffff;
    for (int j = lane; j < hms; j += 64) {
        const double v = f[j];
        if (v < fmin || imin == 0x7fffffff) {
            fmin = v;
            imin = j;
        }
        if (v > fmax || imax == 0x7fffffff) {
            fmax = v;
            imax = j;
        }
        sum += v;
    }
    wave_argmin(fmin, imin);
    wave_argmax(fmax, imax);
    const double mean = group_sum<64>(sum) / hms;
    double m2 = 0.;
    for (int j = lane; j < hms; j += 64) {
        const double dv = f[j] - mean;
        m2 += dv * dv;
    }
    m2 = group_sum<64>(m2);
    s.fstd = sqrt(m2 / hms);
    s.fbest = fmin;
    s.ibest = imin;
    s.fworst = fmax;
    s.iworst = imax;
    s.wide = s.fstd > fstdmin ? 1 : 0;
    s.conv = 0;
}

// :60-74 for the populations p0 .. p0 + gridDim.x - 1; also what follows a set of "x" or "f".
// NSHS_INIT_DRAW: uniform rows; NSHS_INIT_EVAL: their values, a wavefront per row; then, always,
// the statistics.  grid (populations), 256 threads
__global__ __launch_bounds__(256) void nshs_init(NshsDev d, NshsConst c, int p0, int mode)
{
#pragma clang fp contract(off)
    const int p = p0 + blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = c.n, hms = c.hms;
    double *fv = d.f + (size_t) p * hms;
    for (int r = wave; r < hms; r += 4) {
        double *x = d.X + ((size_t) p * hms + r) * c.ld;
        if (mode & NSHS_INIT_DRAW) {
            for (int j = lane; j < n; j += 64) {
                const u32x4 w = philox4x32_10(c.seed, (uint32_t) r, (uint32_t) j, 0,
                        stream_word(STREAM_INIT, (uint32_t) p));
                x[j] = nshs_between(u01(w.x, w.y), d.lower[j], d.upper[j]);
            }
            wave_sync();
        }
        if (mode & NSHS_INIT_EVAL) {
            double f = eval_row_group<64>(c.obj, n, x, d.aux, lane);
            if (f != f) f = NSHS_INF;
            if (lane == 0) fv[r] = f;
        }
    }
    __syncthreads();
    if (wave != 0) return;
    NshsScal s = d.scal[p];
    nshs_select(fv, hms, lane, c.fstdmin, s);
    if (lane == 0) d.scal[p] = s;
}

// :112-147: a thread per coordinate.  grid (P), 256 threads
__global__ __launch_bounds__(256) void nshs_generate(NshsDev d, NshsConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    const NshsScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const double *hm = d.X + (size_t) p * c.hms * c.ld;
    const int wide = sc->wide, it = sc->it;
    for (int i = threadIdx.x; i < c.n; i += 256) {
        double u0, u1, u2, u3;
        nshs_uniforms(d, c, p, i, it, u0, u1, u2, u3);
        d.cand[(size_t) p * c.ld + i] = nshs_coordinate(c, hm, d.lower[i], d.upper[i], i, wide, it, u0, u1, u2, u3);
    }
}

// :150: one wavefront per population.  grid (P), 64 threads
__global__ __launch_bounds__(64) void nshs_eval(NshsDev d, NshsConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    if (pop_frozen(c, d.scal + p)) return;
    double f = eval_row_group<64>(c.obj, c.n, d.cand + (size_t) p * c.ld, d.aux, threadIdx.x);
    if (f != f) f = NSHS_INF;
    if (threadIdx.x == 0) d.fcand[p] = f;
}

// :157-169, :96, :151: the candidate against the worst row (strict <), the statistics when the
// memory changed (they are functions of f alone), the counters and the budget.
// grid (P), 64 threads
__global__ __launch_bounds__(64) void nshs_replace(NshsDev d, NshsConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x, lane = threadIdx.x;
    if (pop_frozen(c, d.scal + p)) return;
    NshsScal s = d.scal[p];
    double *fv = d.f + (size_t) p * c.hms;
    const double fc = d.fcand[p];
    s.accepted = fc < s.fworst ? 1 : 0;
    if (s.accepted) {
        double *row = d.X + ((size_t) p * c.hms + s.iworst) * c.ld;
        const double *cand = d.cand + (size_t) p * c.ld;
        for (int i = lane; i < c.n; i += 64) row[i] = cand[i];
        if (lane == 0) fv[s.iworst] = fc;
        wave_sync();
        nshs_select(fv, c.hms, lane, c.fstdmin, s);
    }
    s.it++;
    s.fev++;
    if (s.fev >= c.mfev) s.stop = 2;
    if (lane == 0) d.scal[p] = s;
}

// the hand-over point of nshs_steps' T threads
template<int T>
__device__ inline void nshs_sync()
{
    if (T == 64) wave_sync();
    else __syncthreads();
}

// The hot path: K whole iterations of one population per launch.  One workgroup of T threads per
// population; the lanes run over the coordinates for the draws, the gather and the clamp, then the
// first wavefront evaluates the candidate from LDS (eval_row_group<64>: the sum nshs_eval forms),
// holds it against the worst value, and when the memory changes recomputes its statistics.
// HM_LDS: the memory and its values were read into LDS at the start of the launch, an accepted
// candidate is written to its LDS row and through to its global row, so only the scalars and the
// last candidate are left to write at the end.  Otherwise the same body gathers from and writes to
// global memory (its own writes are ordered before its reads by the hand-over points).  The
// iteration's branch, its counter word and the budget live in registers: a population that reaches
// fev == mfev sets stop = 2 and leaves the loop.
// LDS: cand, lower, upper [ld] each, then (HM_LDS) f [hms] and the memory [hms][ld].  grid (P), T threads
template<int T, bool HM_LDS>
__global__ __launch_bounds__(T) void nshs_steps(NshsDev d, NshsConst c, int K)
{
#pragma clang fp contract(off)
    extern __shared__ double nshs_lds[];
    __shared__ int bc_acc, bc_row, bc_wide;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int n = c.n, ld = c.ld, hms = c.hms;
    NshsScal s = d.scal[p];
    if (pop_frozen(c, &s)) return;
    double *gx = d.X + (size_t) p * hms * ld, *gf = d.f + (size_t) p * hms;
    double *cand = nshs_lds, *lo = cand + ld, *up = lo + ld;
    double *fv, *hm;
    for (int i = tid; i < n; i += T) {
        lo[i] = d.lower[i];
        up[i] = d.upper[i];
    }
    if constexpr (HM_LDS) {
        fv = up + ld;
        hm = fv + hms;
        for (int q = tid; q < hms * ld; q += T) hm[q] = gx[q];
        for (int q = tid; q < hms; q += T) fv[q] = gf[q];
    } else {
        fv = gf;
        hm = gx;
    }
    nshs_sync<T>();
    double fcand = d.fcand[p];
    int done = 0;
    for (int k = 0; k < K; k++) {
        if (c.honor_stop && s.stop) break;
        for (int i = tid; i < n; i += T) {
            double u0, u1, u2, u3;
            nshs_uniforms(d, c, p, i, s.it, u0, u1, u2, u3);
            cand[i] = nshs_coordinate(c, hm, lo[i], up[i], i, s.wide, s.it, u0, u1, u2, u3);
        }
        nshs_sync<T>();
        int acc = 0, row = s.iworst;
        if (tid < 64) {
            double fc = eval_row_group<64>(c.obj, n, cand, d.aux, lane);
            if (fc != fc) fc = NSHS_INF;
            fcand = fc;
            acc = fc < s.fworst ? 1 : 0;
            s.accepted = acc;
            if (acc) {
                if (lane == 0) {
                    fv[row] = fc;
                    if (HM_LDS) gf[row] = fc;
                }
                wave_sync();
                nshs_select(fv, hms, lane, c.fstdmin, s);
            }
            if (T > 64 && tid == 0) {
                bc_acc = acc;
                bc_row = row;
                bc_wide = s.wide;
            }
        }
        if (T > 64) {
            __syncthreads();
            acc = bc_acc;
            row = bc_row;
            s.wide = bc_wide;
        }
        if (acc) {
            for (int i = tid; i < n; i += T) {
                const double v = cand[i];
                hm[(size_t) row * ld + i] = v;
                if (HM_LDS) gx[(size_t) row * ld + i] = v;
            }
        }
        nshs_sync<T>();
        s.it++;
        s.fev++;
        if (s.fev >= c.mfev) s.stop = 2;
        done++;
    }
    if (!done) return;
    for (int i = tid; i < n; i += T) d.cand[(size_t) p * ld + i] = cand[i];
    if (tid == 0) {
        d.fcand[p] = fcand;
        d.scal[p] = s;
    }
}

} // namespace bbo
