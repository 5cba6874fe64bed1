// bbo_rosen_kernels.hpp -- Rosenbrock's rotating-axes search as gfx950 kernels.
//
//   kernel       reference lines (rosenbrock.cpp)                     work per population
//   rosen_walk   :227-332 lineSearch(), :95-210 iterate()             searches of about 8 evaluations; n^2 sums
//   rosen_eval   the values of a pending batch with a built-in (bbo_rosen_phase 1)   up to 4 rows
//
// A thread owns the coordinates tid, tid + threads, ...: every daxpy1 / daxpym / dscal1 of the reference is the
// same expression per coordinate.  The comparisons of the search, dnrm2 (in its scaled form) and the sum of
// the step test are the reference's sequential folds, the same in every thread.  The n^2 sums of Palmer's
// orthogonalisation are independent of each other and spread over all threads, each summed with jj ascending as
// the reference sums it.  Nothing is contracted into a fused multiply-add.
#pragma once

#include "bbo_rosen.hpp"
#include "bbo_objectives.hpp"
#include "bbo_wave.hpp"

namespace bbo {

#define ROSEN_INF (__builtin_huge_val())

// a built-in at one row, by one wavefront; a NaN counts as +inf
__device__ inline double rosen_value(const RosenConst &c, const double *row, const double *aux, int lane)
{
    const double f = eval_row_group<64>(c.obj, c.n, row, aux, lane);
    return f != f ? ROSEN_INF : f;
}

#ifndef BBO_WALK_DEVICE_FUNCTIONS_ONLY   // (bbo_bh.hip takes the value function and the re-arm, not the kernels)
// grid (P), 64 threads (the narrow form: the points of a batch in turn) or ROSEN_THREADS (the wide form: a
// wavefront per point of a batch)
//   mode   ROSEN_FUSED: evaluates inside and ends at the goal or a stop.  ROSEN_ADVANCE: walks to the next batch
//          of points, leaves them in `cand` and ends.  ROSEN_ABSORB: takes d.value for the pending batch, then
//          advances.
//   begin  the goal becomes `it + K` first
// c.honor_stop (bbo_run): a population that converged or spent its budget starts no further search.
__global__ __launch_bounds__(ROSEN_THREADS) void rosen_walk(RosenDev d, RosenConst c, int mode, int K, int begin)
{
#pragma clang fp contract(off)
    __shared__ double x0s[ROSEN_MAX_N], xs[ROSEN_MAX_N], vr[ROSEN_MAX_N];
    __shared__ double ia[ROSEN_MAX_N], ic[ROSEN_MAX_N], id[ROSEN_MAX_N], tmpv[ROSEN_MAX_N];
    __shared__ double ds[ROSEN_MAX_N + 2], temps[ROSEN_MAX_N + 2], vals[ROSEN_BATCH];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nt = blockDim.x;
    const int n = c.n, ld = c.ld;
    const bool wide = nt > 64;
    RosenScal s = d.scal[p];
    if (pop_frozen(c, &s)) return;
    if (mode == ROSEN_ABSORB && !s.pending) return;
    if (mode == ROSEN_ADVANCE && s.pending) return;
    if (begin) s.goal = s.it + K;
    if (s.stage == ROSEN_IDLE && s.it >= s.goal) return;

    const long long t_begin = wall_clock64();
    const size_t pv = (size_t) p * ld;
    double *X = d.x + (size_t) p * (n + 2) * ld;
    double *V = d.v + (size_t) p * (n + 2) * ld;
    double *VO = d.vold + (size_t) p * (n + 2) * ld;
    double *cand = d.cand + (size_t) p * ROSEN_BATCH * ld;
    for (int q = tid; q < n + 2; q += nt) ds[q] = d.d[(size_t) p * (n + 2) + q];
    if (s.stage != ROSEN_IDLE)
        for (int j = tid; j < n; j += nt) {
            x0s[j] = d.x0[pv + j];
            xs[j] = X[(size_t) s.i * ld + j];
            vr[j] = V[(size_t) s.i * ld + j];
        }
    if (mode == ROSEN_ABSORB) {
        if (tid < s.pending) vals[tid] = d.value[(size_t) p * ROSEN_BATCH + tid];
        s.pending = 0;
    }

    // daxpy1 (blas.cpp:75) per coordinate: x0 + da v, the copy of x0 where da == 0
    auto axpy = [&](double *dst, double da) {
        for (int j = tid; j < n; j += nt) dst[j] = da == 0. ? x0s[j] : x0s[j] + da * vr[j];
    };
    // The batch pt[0 .. cnt): evaluated here (the wide form a wavefront per point, the narrow form in turn) or
    // left pending in `cand`.  True: the launch ends.
    auto submit = [&](int cnt, const double *p0, const double *p1, const double *p2, const double *p3) {
        const double *pt[ROSEN_BATCH] = { p0, p1, p2, p3 };
        __syncthreads();
        if (mode != ROSEN_FUSED) {
            for (int k = 0; k < cnt; k++)
                for (int j = tid; j < n; j += nt) cand[(size_t) k * ld + j] = pt[k][j];
            s.pending = cnt;
            return true;
        }
        // (the four interpolation points stay readable next to fs: "cand")
        if (cnt == ROSEN_BATCH)
            for (int k = 0; k < cnt; k++)
                for (int j = tid; j < n; j += nt) cand[(size_t) k * ld + j] = pt[k][j];
        if (wide) {
            if (w < cnt) {
                const double f = rosen_value(c, pt[w], d.aux, lane);
                if (lane == 0) vals[w] = f;
            }
        } else {
            for (int k = 0; k < cnt; k++) {
                const double f = rosen_value(c, pt[k], d.aux, lane);
                if (lane == 0) vals[k] = f;
            }
        }
        return false;
    };

    for (;;) {
        __syncthreads();
        if (s.stage == ROSEN_IDLE) {
            if (s.it >= s.goal || (c.honor_stop && s.stop)) break;
            for (int j = tid; j < n; j += nt) {                       // :230-237
                x0s[j] = X[(size_t) (s.i - 1) * ld + j];
                vr[j] = V[(size_t) s.i * ld + j];
            }
            s.s = s.stepi;
            s.fs[0] = s.fs[1] = s.fs[2] = s.fs[3] = 0.;
            s.pdir = ROSEN_FORWARD;
            s.prounds = 0;
            s.pimin = -1;
            s.pend = ROSEN_END_NONE;
            axpy(xs, s.s);
            s.stage = ROSEN_WAIT_FIRST;
            if (submit(2, x0s, xs, nullptr, nullptr)) break;
            continue;
        }
        if (s.stage == ROSEN_WAIT_FIRST) {                             // :233-251
            s.fx0 = vals[0];
            s.fx = vals[1];
            s.fev += 2;
            if (s.fx > s.fx0) {
                const double da = -2. * s.s;                        // daxpym
                if (da != 0.)
                    for (int j = tid; j < n; j += nt) xs[j] = xs[j] + da * vr[j];
                s.s = -s.s;
                s.pdir = ROSEN_BACKWARD;
                s.stage = ROSEN_WAIT_BACK;
                if (submit(1, xs, nullptr, nullptr, nullptr)) break;
                continue;
            }
            s.stage = ROSEN_NEXT_DOUBLE;
        }
        if (s.stage == ROSEN_WAIT_BACK) {
            s.fx = vals[0];
            s.fev++;
            if (s.fx > s.fx0) {
                s.pdir = ROSEN_STRAIGHT;
                s.stage = ROSEN_PREP_INTERP;
            } else {
                s.stage = ROSEN_NEXT_DOUBLE;
            }
        }
        if (s.stage == ROSEN_WAIT_DOUBLE) {                            // :259-264
            s.fx = vals[0];
            s.fev++;
            s.prounds++;
            if (s.fev > c.mfev) {                                     // :261, :103-109
                s.pend = ROSEN_END_BUDGET;
                for (int j = tid; j < n; j += nt) X[(size_t) s.i * ld + j] = xs[j];
                if (tid == 0) ds[s.i] = s.s;
                s.stop = 2;
                s.it++;
                s.stage = ROSEN_IDLE;
                continue;
            }
            if (s.fx <= s.fx0 && fabs(s.s) < 1e30) {
                s.stage = ROSEN_NEXT_DOUBLE;
            } else {
                s.s /= 2.;
                s.stage = ROSEN_PREP_INTERP;
            }
        }
        if (s.stage == ROSEN_NEXT_DOUBLE) {                            // :255-258
            s.s *= 2.;
            for (int j = tid; j < n; j += nt) x0s[j] = xs[j];
            s.fx0 = s.fx;
            axpy(xs, s.s);
            s.stage = ROSEN_WAIT_DOUBLE;
            if (submit(1, xs, nullptr, nullptr, nullptr)) break;
            continue;
        }
        if (s.stage == ROSEN_PREP_INTERP) {                            // :272-279
            axpy(ia, -s.s);
            axpy(ic, s.s);
            axpy(id, 2. * s.s);
            s.stage = ROSEN_WAIT_INTERP;
            // (x0 is evaluated again, as in the reference)
            if (submit(4, ia, x0s, ic, id)) break;
            continue;
        }
        if (s.stage == ROSEN_WAIT_INTERP) {                            // :280-318
            for (int k = 0; k < 4; k++) s.fs[k] = vals[k];
            s.fev += 4;
            int imin = 0;
            for (int k = 1; k < 4; k++)
                if (s.fs[k] < s.fs[imin]) imin = k;
            s.pimin = imin;
            if (imin == 1 || imin == 2) {
                const double num = s.s * (s.fs[imin - 1] - s.fs[imin + 1]);
                const double den = 2. * (s.fs[imin - 1] - 2. * s.fs[imin] + s.fs[imin + 1]);
                double stepf = imin == 1 ? 0. : s.s;
                if (fabs(den) > 0.) stepf += num / den;
                s.stepf = stepf;
                __syncthreads();
                axpy(xs, stepf);
                s.stage = ROSEN_WAIT_FINAL;
                if (submit(1, xs, nullptr, nullptr, nullptr)) break;
                continue;
            }
            s.stepf = imin == 0 ? -s.s : 2. * s.s;
            __syncthreads();
            axpy(xs, s.stepf);
            s.s = s.stepf;
            s.stage = ROSEN_FINISH;
        }
        if (s.stage == ROSEN_WAIT_FINAL) {                             // :317-331
            s.fx = vals[0];
            s.fev++;
            s.pend = ROSEN_END_KEPT;
            if (s.fx > s.fs[s.pimin]) {
                s.stepf = s.pimin == 1 ? 0. : s.s;
                __syncthreads();
                axpy(xs, s.stepf);
                s.pend = ROSEN_END_RESTORED;
            }
            s.s = s.stepf;
            s.stage = ROSEN_FINISH;
        }
        if (s.stage != ROSEN_FINISH) continue;

        // iterate() behind the search (:103-210)
        const int i = s.i;
        for (int j = tid; j < n; j += nt) X[(size_t) i * ld + j] = xs[j];
        if (tid == 0) ds[i] = s.s;
        s.it++;
        s.orth = 0;
        s.stage = ROSEN_IDLE;
        __syncthreads();
        if (i < n) {                                                   // :112-115
            s.i++;
            continue;
        }
        if (i == n) {                                                  // :118-130
            for (int j = tid; j < n; j += nt) tmpv[j] = X[(size_t) n * ld + j] + -1. * X[j];
            __syncthreads();
            double zn;                                                 // dnrm2 (blas.cpp:154)
            if (n == 1) {
                zn = fabs(tmpv[0]);
            } else {
                double scale = 0., ssq = 1.;
                for (int j = 0; j < n; j++)
                    if (tmpv[j] != 0.) {
                        const double a = fabs(tmpv[j]);
                        if (scale < a) {
                            ssq = 1. + ssq * (scale / a) * (scale / a);
                            scale = a;
                        } else {
                            ssq = ssq + (a / scale) * (a / scale);
                        }
                    }
                zn = scale * sqrt(ssq);
            }
            if (zn > 0.) {
                const double da = 1. / zn;
                for (int j = tid; j < n; j += nt) V[(size_t) (n + 1) * ld + j] = tmpv[j] * da;
                s.i = n + 1;
                continue;
            }
            for (int j = tid; j < n; j += nt) X[(size_t) (n + 1) * ld + j] = X[(size_t) n * ld + j];
            if (tid == 0) ds[n + 1] = 0.;
        } else {                                                       // :134-191
            for (int j = tid; j < n; j += nt) {
                const double t = X[(size_t) (n + 1) * ld + j] - X[j];
                tmpv[j] = t * t;
            }
            __syncthreads();
            double dxn = 0.;
            for (int j = 0; j < n; j++) dxn += tmpv[j];
            dxn = sqrt(dxn);
            if (dxn >= s.stepi) {
                const long long t_orth = wall_clock64();
                for (int q = tid; q < n * ld; q += nt) VO[ld + q] = V[ld + q];
                if (tid == 0)
                    for (int j = n; j >= 1; j--) temps[j] = j == n ? ds[j] * ds[j] : temps[j + 1] + ds[j] * ds[j];
                __syncthreads();
                // Palmer (:162-185): the sum of (ii, j) over jj = ii .. n ascending, a thread per sum
                for (int q = tid; q < n * n; q += nt) {
                    const int ii = q / n + 1, j = q - (ii - 1) * n;
                    if (temps[ii] <= 0.) continue;
                    double a = 0.;
                    for (int jj = ii; jj <= n; jj++) a += ds[jj] * VO[(size_t) jj * ld + j];
                    if (ii == 1) {
                        a /= sqrt(temps[1]);
                    } else {
                        a *= ds[ii - 1];
                        a -= VO[(size_t) (ii - 1) * ld + j] * temps[ii];
                        a /= sqrt(temps[ii] * temps[ii - 1]);
                    }
                    V[(size_t) ii * ld + j] = a;
                }
                __syncthreads();
                if (tid == 0) ds[1] = ds[n + 1];
                for (int j = tid; j < n; j += nt) {
                    X[j] = X[(size_t) n * ld + j];
                    X[ld + j] = X[(size_t) (n + 1) * ld + j];
                }
                s.i = 2;
                s.orth = 1;
                s.orths++;
                s.orth_ticks += wall_clock64() - t_orth;
                continue;
            }
        }
        s.stepi *= c.decf;                                             // :195-209
        if (s.stepi <= c.tol) {
            for (int j = tid; j < n; j += nt) d.x1[pv + j] = X[(size_t) (n + 1) * ld + j];
            s.stop = 1;
            s.conv = 1;
            continue;
        }
        for (int j = tid; j < n; j += nt) X[j] = X[(size_t) (n + 1) * ld + j];
        s.i = 1;
        if (s.fev >= c.mfev) s.stop = 2;
    }

    __syncthreads();
    if (s.stage != ROSEN_IDLE)
        for (int j = tid; j < n; j += nt) {
            d.x0[pv + j] = x0s[j];
            X[(size_t) s.i * ld + j] = xs[j];
        }
    for (int q = tid; q < n + 2; q += nt) d.d[(size_t) p * (n + 2) + q] = ds[q];
    s.walk_ticks += wall_clock64() - t_begin;
    if (tid == 0) d.scal[p] = s;
}
#endif

// A fresh start of population p at `from` (n doubles), by the workgroup that calls it: exactly the state init()
// uploads -- row 0 of x = from and its other rows zero, v the identity in rows 1 .. n, vold, d, x0 and x1 zero
// (x1 is what a budget exit returns), the fresh scalars (stepi = step0, i = 1, pimin = -1, the counters and stop
// zero).  cand and value are written by the walk before it reads them (BasinHopping's hops).
__device__ inline void rosen_rearm(const RosenDev &d, const RosenConst &c, int p, const double *from, int tid, int nt)
{
    const int n = c.n, ld = c.ld;
    const size_t pv = (size_t) p * ld, pm = (size_t) p * (n + 2) * ld;
    for (int q = tid; q < (n + 2) * ld; q += nt) {
        const int r = q / ld, j = q - r * ld;
        d.x[pm + q] = r == 0 && j < n ? from[j] : 0.;
        d.v[pm + q] = r >= 1 && r <= n && j == r - 1 ? 1. : 0.;
        d.vold[pm + q] = 0.;
    }
    for (int q = tid; q < n + 2; q += nt) d.d[(size_t) p * (n + 2) + q] = 0.;
    for (int j = tid; j < ld; j += nt) {
        d.x0[pv + j] = 0.;
        d.x1[pv + j] = 0.;
    }
    if (tid == 0) d.scal[p] = rosen_fresh_scal(c.step0);
}

#ifndef BBO_WALK_DEVICE_FUNCTIONS_ONLY
// the built-in at every population's pending batch (bbo_rosen_phase 1).  grid (P), ROSEN_THREADS threads
__global__ __launch_bounds__(ROSEN_THREADS) void rosen_eval(RosenDev d, RosenConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const RosenScal *sc = d.scal + p;
    if (!sc->pending || pop_frozen(c, sc)) return;
    if (w >= sc->pending) return;
    const double f = rosen_value(c, d.cand + ((size_t) p * ROSEN_BATCH + w) * c.ld, d.aux, lane);
    if (lane == 0) d.value[(size_t) p * ROSEN_BATCH + w] = f;
}
#endif

} // namespace bbo
