// bbo_acd_kernels.hpp -- ACD as gfx950 kernels.
//
//   kernel       reference lines (acd.cpp)                                   work per population
//   acd_init     :104-115 B = invB = C = I, diagd = colmax = 1              n values
//   acd_sweep    :122-162, :176-177 coordinate steps; :204-228 the stop test  up to n steps of 2 evaluations
//   acd_eval     :131-132 the values of a host-driven step's two points      two rows
//   acd_ae       :167-170 the ranking, :236-284 m, mold, artmp, p, C         O(n^2), sequential chains per lane
//   acd_post     :317-332 roots, invB, B; colmax; :174; the stop test        O(n^2)
// The decomposition between acd_ae and acd_post is the project's eigensolver (bbo_eig.hpp), launched by
// the host over a view of Cw, V and Dv.
#pragma once

#include "bbo_acd.hpp"
#include "bbo_cma.hpp"
#include "bbo_objectives.hpp"
#include "bbo_wave.hpp"

namespace bbo {

#define ACD_INF (__builtin_huge_val())

// std::max(a, b) and std::min(a, b) with their treatment of a NaN: the first argument unless the
// comparison holds
__device__ inline double acd_max(double a, double b) { return a < b ? b : a; }
__device__ inline double acd_min(double a, double b) { return b < a ? b : a; }

// grid (P), ACD_THREADS threads: the identities of a fresh run (the buffers are zero)
__global__ __launch_bounds__(ACD_THREADS) void acd_init(AcdDev d, AcdConst c)
{
    const int p = blockIdx.x, i = threadIdx.x, ld = c.ld;
    if (i >= c.n) return;
    const size_t mat = (size_t) p * ld * ld + (size_t) i * ld + i;
    d.Bt[mat] = 1.;
    d.invBt[mat] = 1.;
    d.C[mat] = 1.;
    d.diagd[(size_t) p * ld + i] = 1.;
    d.colmax[(size_t) p * ld + i] = 1.;
}

// converged() (:204-228) behind a step, the same value in every thread; 0: not converged, 1: the history
// rule, 2: the step rule.  `it` has been advanced, so the newest entry of the ring, fhist[(it - 1) % cp],
// is the f_best this step wrote: s.fbest.  The oldest, fhist[it % cp], was written cp - 1 steps ago, by
// an earlier launch (a launch ends with its sweep and cp > n).
// The reference's step rule takes max over ix and i of |sigma[ix] B[i][ix]|: n^2 products per step.  Here
// colmax[ix] = max_i |B[i][ix]| is kept from the last update and the test is max_ix sigma[ix] colmax[ix].
// That is the reference's value exactly: |sigma b| = sigma |b| for sigma >= 0, and a rounded product
// with a non-negative factor is monotone in the other factor, so the largest |b| of a column gives its
// largest product.  A NaN product (inf times 0) is passed over by std::max in either form, and sigma stays
// non-negative because it starts as (upper - lower) / 4 of an ordered box and is only ever scaled.
__device__ inline int acd_converged(const AcdConst &c, const AcdScal &s, const double *fhist,
        const double *sig, const double *cm)
{
#pragma clang fp contract(off)
    if (s.it > c.cp) {
        const double f0 = s.fbest;
        const double f1 = fhist[s.it % c.cp];
        if (fabs(f1 - f0) < c.ftol) return 1;
    }
    double dxmax = 0.;
    for (int j = threadIdx.x & 63; j < c.n; j += 64) dxmax = acd_max(dxmax, fabs(sig[j] * cm[j]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dxmax = acd_max(dxmax, __shfl_xor(dxmax, off, 64));
    return dxmax < c.xtol ? 2 : 0;
}

// what follows converged() in optimize()'s loop (:188-194)
__device__ inline void acd_stop(const AcdConst &c, AcdScal &s, int rule)
{
    s.conv = rule ? 1 : 0;
    s.rule = rule;
    if (!s.stop) {
        if (rule) s.stop = 1;
        else if (s.fev >= c.mfev) s.stop = 2;
    }
}

// The hot path.  One workgroup of two wavefronts per population: wavefront 0 forms and evaluates x1,
// wavefront 1 x2, both from x_best in LDS; the lanes own the coordinates.  Everything a later launch
// needs is in AcdScal and the population's vectors, so a launch cut after any step resumes with the
// same bits.
//   mode   ACD_FUSED: evaluates inside; ends at the goal, at the end of the sweep, at a stop and where an
//          update is due.  ACD_ADVANCE: forms x1 and x2 into cand and ends.  ACD_ABSORB: takes
//          d.value for them and completes that one step.
//   begin  the goal becomes `it + K` first
// grid (P), ACD_THREADS threads
__global__ __launch_bounds__(ACD_THREADS) void acd_sweep(AcdDev d, AcdConst c, int mode, int K, int begin)
{
#pragma clang fp contract(off)
    __shared__ double xs[2][ACD_MAX_N], xb[ACD_MAX_N], sig[ACD_MAX_N], cm[ACD_MAX_N], lo[ACD_MAX_N], up[ACD_MAX_N];
    __shared__ double fv[2];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = c.n, ld = c.ld;
    AcdScal s = d.scal[p];
    if (pop_frozen(c, &s)) return;
    if (mode == ACD_ABSORB && !s.pending) return;
    if (mode == ACD_ADVANCE && s.pending) return;
    if (begin) s.goal = s.it + K;
    const size_t pv = (size_t) p * ld;
    const double *Bt = d.Bt + (size_t) p * ld * ld;
    double *X = d.X + (size_t) p * 2 * n * ld, *fa = d.f + (size_t) p * 2 * n;
    double *fhist = d.fhist + (size_t) p * c.cp;
    double *cand = d.cand + (size_t) p * 2 * ld;
    if (tid < n) {
        xb[tid] = d.xbest[pv + tid];
        sig[tid] = d.sigma[pv + tid];
        cm[tid] = d.colmax[pv + tid];
        lo[tid] = d.lower[tid];
        up[tid] = d.upper[tid];
        if (mode == ACD_ABSORB) {
            xs[0][tid] = cand[tid];
            xs[1][tid] = cand[ld + tid];
        }
    }
    __syncthreads();

    for (;;) {
        if (s.due || s.it >= s.goal || (c.honor_stop && s.stop)) break;
        const int ix = s.ix;
        if (mode != ACD_ABSORB) {       // :125-130
            const double sg = sig[ix];
            for (int i = lane; i < n; i += 64) {
                const double dx = sg * Bt[(size_t) ix * ld + i];
                const double v = w == 0 ? xb[i] - dx : xb[i] + dx;
                xs[w][i] = acd_max(lo[i], acd_min(v, up[i]));
            }
            if (mode == ACD_ADVANCE) {
                for (int i = lane; i < n; i += 64) cand[(size_t) w * ld + i] = xs[w][i];
                s.pending = 1;
                break;
            }
            wave_sync();
            double f = eval_row_group<64>(c.obj, n, xs[w], d.aux, lane);
            if (f != f) f = ACD_INF;
            if (lane == 0) fv[w] = f;
        }
        __syncthreads();
        const double f1 = mode == ACD_ABSORB ? d.value[2 * p] : fv[0];
        const double f2 = mode == ACD_ABSORB ? d.value[2 * p + 1] : fv[1];
        // :136-144: x1, then x2 against the f_best x1 may have left
        const bool success = f1 < s.fbest || f2 < s.fbest;
        int win = 0;
        if (f1 < s.fbest) {
            win = 1;
            s.fbest = f1;
        }
        if (f2 < s.fbest) {
            win = 2;
            s.fbest = f2;
        }
        if (win && tid < n) xb[tid] = xs[win - 1][tid];
        if (tid == 0) {
            fhist[s.it % c.cp] = s.fbest;                           // :147
            sig[ix] *= success ? c.ksucc : c.kunsucc;               // :150-155
        }
        if (success) s.improved = 1;
        for (int i = lane; i < n; i += 64) X[(size_t) (2 * ix + w) * ld + i] = xs[w][i];     // :158-161
        if (lane == 0) fa[2 * ix + w] = w == 0 ? f1 : f2;
        s.fev += 2;
        s.pending = 0;
        const bool last = ix == n - 1;
        s.ix = last ? 0 : ix + 1;                                   // :176-177
        s.it++;
        __syncthreads();
        if (last && s.improved) {
            // :164-175 is acd_ae, the decomposition and acd_post; converged() reads the new B, so the
            // stop test of this step is acd_post's
            s.due = ACD_DUE_AE;
            break;
        }
        acd_stop(c, s, acd_converged(c, s, fhist, sig, cm));
        if (mode == ACD_ABSORB || last) break;
    }

    if (tid < n) {
        d.xbest[pv + tid] = xb[tid];
        d.sigma[pv + tid] = sig[tid];
    }
    if (tid == 0) {
        d.scal[p] = s;
        if (s.it < s.goal && !(c.honor_stop && s.stop)) d.flags[0] = 1;
        if (s.due) d.flags[1] = 1;
    }
}

// :131-132 for a host-driven step with a built-in objective (bbo_acd_phase 1).  grid (P), 128 threads
__global__ __launch_bounds__(ACD_THREADS) void acd_eval(AcdDev d, AcdConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const AcdScal *sc = d.scal + p;
    if (!sc->pending || pop_frozen(c, sc)) return;
    double f = eval_row_group<64>(c.obj, c.n, d.cand + ((size_t) p * 2 + w) * c.ld, d.aux, lane);
    if (f != f) f = ACD_INF;
    if (lane == 0) d.value[2 * p + w] = f;
}

// The update of a due population up to C.  The archive is ranked stably with respect to the persisting
// `order` (bbo_rank.hpp's convention: equal values keep their places): position k of the old order goes
// to the number of values below its own plus the equal ones in front of it.  The reference's std::sort
// is an insertion sort, hence stable, for 2 n <= 16 elements; beyond that its order on ties is
// unspecified, and this is one of the orders it may produce.
// Every sum runs in the reference's order: lane d adds its coordinate over the ranks 0 .. n - 1, lane i
// walks row i of invB, one thread adds denom.  grid (P), ACD_THREADS threads
__global__ __launch_bounds__(ACD_THREADS) void acd_ae(AcdDev d, AcdConst c)
{
#pragma clang fp contract(off)
    __shared__ double fs[2 * ACD_MAX_N], dm[ACD_MAX_N], pn[ACD_MAX_N], art[ACD_MAX_N];
    __shared__ int ord[2 * ACD_MAX_N], nord[2 * ACD_MAX_N];
    __shared__ double bc;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = c.n, ld = c.ld, n2 = 2 * n;
    AcdScal s = d.scal[p];
    if (pop_frozen(c, &s) || s.due != ACD_DUE_AE) return;
    const size_t pv = (size_t) p * ld;
    const double *X = d.X + (size_t) p * n2 * ld;
    int *order = d.order + (size_t) p * n2;
    for (int k = tid; k < n2; k += ACD_THREADS) {
        ord[k] = order[k];
        nord[k] = ord[k];       // (a NaN never gets here; if one did, the ranks it leaves out keep a valid row)
        fs[k] = d.f[(size_t) p * n2 + k];
    }
    __syncthreads();
    for (int k = tid; k < n2; k += ACD_THREADS) {       // :167-170
        const double fk = fs[ord[k]];
        int r = 0;
        for (int j = 0; j < n2; j++) {
            const double fj = fs[ord[j]];
            r += (fj < fk) || (fj == fk && j < k);
        }
        nord[r] = ord[k];
    }
    __syncthreads();
    for (int k = tid; k < n2; k += ACD_THREADS) order[k] = nord[k];
    const int itae = s.itae + 1;                        // :239
    if (tid < n) {                                      // :241-246, :251-257
        const double wgt = 1. / n;
        const double mo = d.m[pv + tid];
        double acc = 0.;
        for (int i = 0; i < n; i++) acc += X[(size_t) nord[i] * ld + tid] * wgt;
        d.m[pv + tid] = acc;
        if (itae > 1) d.mold[pv + tid] = mo;
        dm[tid] = acc - mo;
    }
    if (itae == 1) {
        if (tid == 0) {
            s.itae = itae;
            s.due = ACD_DUE_POST;
            d.scal[p] = s;
        }
        return;
    }
    __syncthreads();
    const double *invBt = d.invBt + (size_t) p * ld * ld;
    if (tid < n) {                                      // :260-265
        double a = 0.;
        for (int j = 0; j < n; j++) a += invBt[(size_t) j * ld + tid] * dm[j];
        art[tid] = a;
    }
    __syncthreads();
    if (tid == 0) {                                     // :266-267
        double den = 0.;
        for (int i = 0; i < n; i++) den = den + art[i] * art[i];
        bc = den;
    }
    __syncthreads();
    const double denom = bc, cp = c.cpath;
    if (tid < n) {                                      // :268-277
        double pi = d.p[pv + tid];
        if (denom <= 0.) {
            pi *= (1. - cp);
        } else {
            const double factor = sqrt(cp * (2. - cp) * n / denom);
            pi = (1. - cp) * pi + factor * dm[tid];
        }
        pn[tid] = pi;
        d.p[pv + tid] = pi;
    }
    __syncthreads();
    double *C = d.C + (size_t) p * ld * ld, *Cw = d.Cw + (size_t) p * ld * ld;
    const double c1 = c.c1;
    for (int q = tid; q < n * n; q += ACD_THREADS) {    // :280-284, and :290-294 for the eigensolver
        const int i = q / n, j = q - i * n;
        const double v = (1. - c1) * C[(size_t) i * ld + j] + c1 * pn[i] * pn[j];
        C[(size_t) i * ld + j] = v;
        if (j <= i) {
            Cw[(size_t) i * ld + j] = v;
            Cw[(size_t) j * ld + i] = v;
        }
    }
    if (tid == 0) {
        // the eigensolver decomposes where fev - eigenlastev > eigenfreq (0.5 in the view) and sets
        // eigenlastev = fev behind it
        d.eigscal[p].fev = 1;
        d.eigscal[p].eigenlastev = 0;
        s.itae = itae;
        s.due = ACD_DUE_EIG;
        d.scal[p] = s;
    }
}

// Behind the decomposition: :317-332 from V and the roots, the diagonal of C as the repair shifted it
// (the eigensolver shifts the diagonal of its copy by the same amounts, :299-315), colmax, :174, and
// the stop test the sweep left to this kernel.  n = 1 needs no eigensolver: V = 1 and the eigenvalue is
// C itself, with the same repair.  grid (P), ACD_THREADS threads
__global__ __launch_bounds__(ACD_THREADS) void acd_post(AcdDev d, AcdConst c)
{
#pragma clang fp contract(off)
    __shared__ double dd[ACD_MAX_N], sig[ACD_MAX_N], cm[ACD_MAX_N];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = c.n, ld = c.ld;
    AcdScal s = d.scal[p];
    if (pop_frozen(c, &s) || (s.due != ACD_DUE_POST && s.due != ACD_DUE_EIG)) return;
    const size_t pv = (size_t) p * ld, pm = (size_t) p * ld * ld;
    double *Bt = d.Bt + pm, *invBt = d.invBt + pm, *C = d.C + pm;
    const double *Cw = d.Cw + pm, *V = d.V + pm;
    if (s.due == ACD_DUE_EIG) {
        if (n == 1) {
            if (tid == 0) {
                double lam = Cw[0], cd = C[0];
                if (lam <= 0.) {
                    lam = acd_max(lam, 0.);
                    const double shift = lam / 1e14;
                    cd += shift;
                    lam += shift;
                }
                if (lam > 1e14 * lam) {
                    const double shift = lam / 1e14 - lam;
                    cd += shift;
                    lam += shift;
                }
                C[0] = cd;
                const double r = sqrt(lam);
                dd[0] = r;
                Bt[0] = 1. * r;
                invBt[0] = 1. / r;
            }
        } else if (tid < n) {
            dd[tid] = d.Dv[pv + tid];
            C[(size_t) tid * ld + tid] = Cw[(size_t) tid * ld + tid];
        }
        __syncthreads();
        if (n > 1)
            for (int q = tid; q < n * n; q += ACD_THREADS) {
                const int a = q / n, b = q - a * n;
                invBt[(size_t) a * ld + b] = V[(size_t) a * ld + b] / dd[b];   // invB[b][a] = V[a][b] / d[b]
                Bt[(size_t) a * ld + b] = V[(size_t) b * ld + a] * dd[a];      // B[b][a] = V[b][a] d[a]
            }
        __syncthreads();
        if (tid < n) {
            d.diagd[pv + tid] = dd[tid];
            double mx = 0.;
            for (int i = 0; i < n; i++) mx = acd_max(mx, fabs(Bt[(size_t) tid * ld + i]));
            d.colmax[pv + tid] = mx;
            cm[tid] = mx;
        }
    } else if (tid < n) {
        cm[tid] = d.colmax[pv + tid];
    }
    if (tid < n) sig[tid] = d.sigma[pv + tid];
    __syncthreads();
    s.improved = 0;                                     // :174
    s.due = ACD_DUE_NONE;
    acd_stop(c, s, acd_converged(c, s, d.fhist + (size_t) p * c.cp, sig, cm));
    if (tid == 0) d.scal[p] = s;
}

} // namespace bbo
