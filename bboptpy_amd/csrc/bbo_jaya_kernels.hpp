// bbo_jaya_kernels.hpp -- one JAYA generation as gfx950 kernels.
//
//   kernel            reference lines (jaya.cpp)                         bytes per member
//   jaya_seed         :95 xchaos, :102-107 the chaotic initial pool       (one thread: a chain)
//   jaya_init_eval    :109-122 uniform pool, its fitness                  8n written
//   jaya_partition    :225-239 shuffle and lengths, :148-157 best / worst  8 + the 2k rows of bw,
//                     :355-377 the 2 n k steps of the chaotic chain
//   jaya_evolve       :260-338 trial, clamp, evaluate, greedy replacement  8n read (+ 8n written
//                     when the trial wins; bw and the box stay in cache): HBM-bound but for one
//                     Philox call per coordinate
//   jaya_select       :327-330 for a host objective (the trial rows come back with their f)
//   jaya_finish       :166-173, :184-217, :241-252                         16
#pragma once

#include "bbo_jaya.hpp"
#include "bbo_objectives.hpp"
#include "bbo_rng.hpp"

namespace bbo {

#define JAYA_INF (__builtin_huge_val())

enum { JAYA_ORIGINAL = 0, JAYA_LEVY = 1, JAYA_TENT = 2, JAYA_LOGISTIC = 3 };
// what a draw of the control stream is for (counter word 0)
enum { JAYA_CTRL_XCHAOS = 0, JAYA_CTRL_LEN = 1, JAYA_CTRL_ROULETTE = 2, JAYA_CTRL_REDRAW = 3 };

// the redraw guards of the chaotic maps (`while (_xchaos == 0.7) _xchaos = Random::get(0., 1.)`)
__device__ inline double jaya_redraw(const JayaConst &c, JayaScal *sc, int p)
{
    const u32x4 w = philox4x32_10_uniform(c.seed, JAYA_CTRL_REDRAW, (uint32_t) sc->nredraw, 0,
            stream_word(STREAM_JAYA_CTRL, (uint32_t) p));
    sc->nredraw++;
    return u01(w.x, w.y);
}

// sampleLogistic, jaya.cpp:369-377
__device__ inline double jaya_logistic(double x, const JayaConst &c, JayaScal *sc, int p)
{
    while (x == 0.5) x = jaya_redraw(c, sc, p);
    return 4. * x * (1. - x);
}

// sampleTentMap, jaya.cpp:355-367
__device__ inline double jaya_tent(double x, const JayaConst &c, JayaScal *sc, int p)
{
    if (x < 0.7) return x / 0.7;
    while (x == 0.7) x = jaya_redraw(c, sc, p);
    return 10. / 3. * (1. - x);
}

// std::max(lower, std::min(t, upper)) with the reference's treatment of a NaN
__device__ inline double jaya_clamp(double t, double lo, double up)
{
    const double m = up < t ? up : t;
    return lo < m ? m : lo;
}

// xchaos, the slots, the strategy weights; under tent_map the initial pool from the LOGISTIC chain
// (jaya.cpp:102-107).  grid (P), 64 threads
__global__ __launch_bounds__(64) void jaya_seed(JayaDev d, JayaConst c)
{
    const int p = blockIdx.x, tid = threadIdx.x;
    JayaScal *sc = d.scal + p;
    const size_t pb = (size_t) p * c.np;
    for (int i = tid; i < c.np; i += 64) d.occ[pb + i] = i;
    for (int q = tid; q < c.nks; q += 64) {
        d.pstrat[(size_t) p * c.nks + q] = 1.;
        d.perfindex[(size_t) p * c.nks + q] = 0.;
    }
    if (tid != 0) return;
    const u32x4 w = philox4x32_10_uniform(c.seed, JAYA_CTRL_XCHAOS, 0, 0, stream_word(STREAM_JAYA_CTRL, (uint32_t) p));
    double xc = u01(w.x, w.y);
    if (c.mutation == JAYA_TENT)
        for (int i = 0; i < c.np; i++)
            for (int j = 0; j < c.n; j++) {
                xc = jaya_logistic(xc, c, sc, p);
                d.X[(pb + i) * c.ld + j] = d.lower[j] + xc * (d.upper[j] - d.lower[j]);
            }
    sc->xchaos = xc;
}

// a wavefront per member.  grid (ceil(np / 4), P), 256 threads, LDS 4 * ld doubles
__global__ __launch_bounds__(256) void jaya_init_eval(JayaDev d, JayaConst c)
{
    const int p = blockIdx.y;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave, n = c.n, ld = c.ld;
    if (i >= c.np) return;
    const size_t pb = (size_t) p * c.np;
    double *x = d.X + (pb + i) * ld, *row = lds + wave * ld;
    double ssq = 0.;
    for (int j = lane; j < n; j += 64) {
        double v;
        if (c.mutation == JAYA_TENT) {
            v = x[j];
        } else {
            const u32x4 w = philox4x32_10(c.seed, (uint32_t) i, (uint32_t) j, 0,
                    stream_word(STREAM_INIT, (uint32_t) p));
            v = u01(w.x, w.y) * (d.upper[j] - d.lower[j]) + d.lower[j];
            x[j] = v;
        }
        row[j] = v;
        ssq += v * v;
    }
    wave_sync();
    ssq = group_sum<64>(ssq);
    double f = JAYA_INF;
    if (c.obj >= 0) {
        f = eval_row_group<64>(c.obj, n, row, d.aux, lane);
        if (f != f) f = JAYA_INF;
    }
    if (lane == 0) {
        d.f[pb + i] = f;
        d.radius[pb + i] = sqrt(ssq);
    }
}

// divideSubpopulation (jaya.cpp:225-239), the best and the worst member of every sub-population
// (:148-157) and the generation's share of the chaotic chain.  One workgroup per population.
// grid (P), 256 threads
__global__ __launch_bounds__(256) void jaya_partition(JayaDev d, JayaConst c)
{
    const int p = blockIdx.x;
    JayaScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int np = c.np, n = c.n, ld = c.ld, nks = c.nks, k = sc->k, gen = sc->gen;
    const size_t pb = (size_t) p * np;
    int *occ = d.occ + pb, *occ2 = d.occ2 + pb;
    int *len = d.len + (size_t) p * nks, *off = d.off + (size_t) p * (nks + 1);
    int *bwrow = d.bwrow + (size_t) p * nks * 2;
    const uint32_t ctrl = stream_word(STREAM_JAYA_CTRL, (uint32_t) p);
    // Random::shuffle: new slot s takes the occupant of slot perm(s)
    for (int s = tid; s < np; s += 256)
        occ2[s] = occ[cso_perm((uint32_t) s, c.kb, (uint32_t) np, c.seed, (uint32_t) gen,
                stream_word(STREAM_JAYA_PERM, (uint32_t) p))];
    __syncthreads();
    for (int s = tid; s < np; s += 256) occ[s] = occ2[s];
    if (tid == 0) {
        const int base = np / k;
        for (int q = 0; q < k; q++) len[q] = base;
        for (int i = 0; i < np - base * k; i++) {
            const u32x4 w = philox4x32_10_uniform(c.seed, JAYA_CTRL_LEN, (uint32_t) i, (uint32_t) gen, ctrl);
            len[uint_below(w.x, k)]++;
        }
        int o = 0;
        for (int q = 0; q < k; q++) {
            off[q] = o;
            o += len[q];
        }
        off[k] = o;
    }
    // the chain: sub-population-major, then coordinate, then r1 before r2 (the order in which the
    // best members meet sampleTentMap / sampleLogistic in the reference's loop)
    if (tid == 64 && c.mutation >= JAYA_TENT) {
        double xc = sc->xchaos;
        double *ch = d.chaos + (size_t) p * nks * n * 2;
        for (int i = 0; i < 2 * n * k; i++) {
            xc = c.mutation == JAYA_TENT ? jaya_tent(xc, c, sc, p) : jaya_logistic(xc, c, sc, p);
            ch[i] = xc;
        }
        sc->xchaos = xc;
    }
    __syncthreads();
    for (int q = wave; q < k; q += 4) {
        const int s0 = off[q], s1 = off[q + 1];
        double fmin = JAYA_INF, fmax = -JAYA_INF;
        int smin = 0x7fffffff, smax = 0x7fffffff;
        for (int s = s0 + lane; s < s1; s += 64) {
            const double fv = d.f[pb + occ[s]];
            if (fv < fmin || (fv == fmin && s < smin)) {
                fmin = fv;
                smin = s;
            }
            if (fv > fmax || (fv == fmax && s < smax)) {
                fmax = fv;
                smax = s;
            }
        }
        wave_argmin(fmin, smin);
        wave_argmax(fmax, smax);
        if (lane == 0) {
            bwrow[2 * q] = occ[min(smin, np - 1)];
            bwrow[2 * q + 1] = occ[min(smax, np - 1)];
        }
    }
    __syncthreads();
    double *bw = d.bw + (size_t) p * nks * 2 * ld;
    for (int e = tid; e < 2 * k * ld; e += 256) {
        const int r = e / ld, j = e - r * ld;
        bw[(size_t) r * ld + j] = d.X[(pb + bwrow[r]) * ld + j];
    }
}

// A wavefront per member: lanes stride the coordinates.  r1, r2 of coordinate j of row i come from
// the Philox call (i, j, generation); the best member of a sub-population takes them from `chaos`
// under the chaotic mutations.  LEVY: Mantegna's step from two ziggurat normals and one more
// uniform (jaya.cpp:275-286, :346-353).  The trial is formed in the reference's operation order;
// best and worst are read from `bw`, so the replacement in place disturbs no other member.
// grid (ceil(np / 4), P), 256 threads, LDS 4 * ld doubles
template<bool LEVY>
__global__ __launch_bounds__(256) void jaya_evolve(JayaDev d, JayaConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const JayaScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x * 4 + wave, n = c.n, ld = c.ld, nks = c.nks;
    if (s >= c.np) return;
    const int gen = sc->gen, k = sc->k;
    const size_t pb = (size_t) p * c.np;
    const int *off = d.off + (size_t) p * (nks + 1);
    int q = 0, hi = k - 1;                     // the sub-population of slot s
    while (q < hi) {
        const int mid = (q + hi + 1) >> 1;
        if (off[mid] <= s) q = mid;
        else hi = mid - 1;
    }
    const int row = d.occ[pb + s];
    const size_t qb = (size_t) p * nks + q;
    const bool chaotic = c.mutation >= JAYA_TENT && d.bwrow[2 * qb] == row;
    const double *xb = d.bw + 2 * qb * ld, *xw = xb + ld;
    const double *ch = d.chaos + qb * n * 2;
    double *x = d.X + (pb + row) * ld;
    double *tg = d.T ? d.T + (pb + row) * ld : nullptr;
    double *dr = d.draws ? d.draws + (pb + row) * n * c.ndraw : nullptr;
    double *trial = lds + wave * ld;
    const uint32_t swr = stream_word(STREAM_JAYA_R, (uint32_t) p);
    double ssq = 0.;
    for (int j = lane; j < n; j += 64) {
        const double xj = x[j], bj = xb[j], wj = xw[j], ax = fabs(xj);
        const u32x4 w = philox4x32_10(c.seed, (uint32_t) row, (uint32_t) j, (uint32_t) gen, swr);
        double r1 = u01(w.x, w.y), r2 = u01(w.z, w.w);
        double from = xj;
        if (LEVY) {
            double zu, zv, z2, z3;
            normal_quad(c.seed, (uint32_t) row, (uint32_t) j, (uint32_t) gen,
                    stream_word(STREAM_JAYA_LEVY, (uint32_t) p), zig_global_wk(), zu, zv, z2, z3);
            const u32x4 wl = philox4x32_10(c.seed, (uint32_t) row, (uint32_t) j | 0x80000000u,
                    (uint32_t) gen, swr);
            const double ul = u01(wl.x, wl.y);
            const double step = (zu * c.sigmau) / pow(fabs(zv), 1. / c.beta);
            const double step_size = c.scale * step * (xj - bj);
            from = xj + step_size * ul;
            if (dr) {
                dr[j * 5] = zu;
                dr[j * 5 + 1] = zv;
                dr[j * 5 + 2] = ul;
            }
        }
        if (dr) {               // (the Philox pair: the model takes the chain's for a best member)
            dr[j * c.ndraw + c.ndraw - 2] = r1;
            dr[j * c.ndraw + c.ndraw - 1] = r2;
        }
        if (chaotic) {
            r1 = ch[2 * j];
            r2 = ch[2 * j + 1];
        }
        double t = from + r1 * (bj - ax) - r2 * (wj - ax);
        t = jaya_clamp(t, d.lower[j], d.upper[j]);
        trial[j] = t;
        if (tg) tg[j] = t;
        ssq += t * t;
    }
    if (c.obj < 0) return;      // a host objective: jaya_select finishes the member
    wave_sync();
    ssq = group_sum<64>(ssq);
    double ft = eval_row_group<64>(c.obj, n, trial, d.aux, lane);
    if (ft != ft) ft = JAYA_INF;
    const bool take = ft < d.f[pb + row];
    if (take)
        for (int j = lane; j < n; j += 64) x[j] = trial[j];
    if (lane == 0) {
        d.ftrial[pb + row] = ft;
        if (take) {
            d.f[pb + row] = ft;
            d.radius[pb + row] = sqrt(ssq);
        }
    }
}

// greedy replacement from T / ftrial (host objective).  grid (ceil(np / 4), P), 256 threads
__global__ __launch_bounds__(256) void jaya_select(JayaDev d, JayaConst c)
{
    const int p = blockIdx.y;
    if (pop_frozen(c, d.scal + p)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave, n = c.n, ld = c.ld;
    if (row >= c.np) return;
    const size_t pb = (size_t) p * c.np;
    const double ft = d.ftrial[pb + row];
    if (!(ft < d.f[pb + row])) return;
    double *x = d.X + (pb + row) * ld;
    const double *t = d.T + (pb + row) * ld;
    double ssq = 0.;
    for (int j = lane; j < n; j += 64) {
        const double v = t[j];
        x[j] = v;
        ssq += v * v;
    }
    ssq = group_sum<64>(ssq);
    if (lane == 0) {
        d.f[pb + row] = ft;
        d.radius[pb + row] = sqrt(ssq);
    }
}

// the incumbent (on a tie the lowest row), the spread of the radii, the performance index and the
// roulette for the next k, the stop flags in optimize()'s order.  `best`: the reference resets
// _best to +inf and then takes max(_best, f) per member (jaya.cpp:143, :333), so it IS +inf after
// every generation, the improvement -inf after the first and NaN from then on, and the weight of
// the k in use 0 and then NaN: from the third generation on the roulette falls through to
// k = nks.  That arithmetic is kept as it is (the outcome bands of the reference are those of
// k = nks).  grid (P), 256 threads
__global__ __launch_bounds__(256) void jaya_finish(JayaDev d, JayaConst c, int init_only)
{
    const int p = blockIdx.x;
    JayaScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    __shared__ double smin[4], ssum[4];
    __shared__ int srow[4];
    __shared__ int take;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, np = c.np, nks = c.nks;
    const size_t pb = (size_t) p * np;
    double fmin = JAYA_INF, rsum = 0.;
    int rmin = 0x7fffffff;
    for (int i = tid; i < np; i += 256) {
        const double fv = d.f[pb + i];
        if (fv < fmin || (fv == fmin && i < rmin)) {
            fmin = fv;
            rmin = i;
        }
        rsum += d.radius[pb + i];
    }
    wave_argmin(fmin, rmin);
    rsum = group_sum<64>(rsum);
    if (lane == 0) {
        smin[wave] = fmin;
        srow[wave] = rmin;
        ssum[wave] = rsum;
    }
    __syncthreads();
    fmin = smin[0];
    rmin = srow[0];
    for (int w = 1; w < 4; w++) {
        if (smin[w] < fmin || (smin[w] == fmin && srow[w] < rmin)) {
            fmin = smin[w];
            rmin = srow[w];
        }
    }
    const double mean = ((ssum[0] + ssum[1]) + (ssum[2] + ssum[3])) / np;
    double m2 = 0.;
    for (int i = tid; i < np; i += 256) {
        const double dd = d.radius[pb + i] - mean;
        m2 += dd * dd;
    }
    m2 = group_sum<64>(m2);
    __syncthreads();
    if (lane == 0) ssum[wave] = m2;
    if (tid == 0) take = fmin < sc->fgbest && rmin < np ? 1 : 0;
    __syncthreads();
    m2 = (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]);
    if (take)
        for (int j = tid; j < c.ld; j += 256) d.bestx[(size_t) p * c.ld + j] = d.X[(pb + rmin) * c.ld + j];
    if (tid != 0) return;
    if (take) sc->fgbest = fmin;
    sc->m2 = m2;
    const int conv = m2 <= (np - 1) * c.tol * c.tol ? 1 : 0;
    sc->conv = conv;
    if (init_only) {
        sc->best = sc->fgbest;      // jaya.cpp:124
        return;
    }
    const int gen = sc->gen, k = sc->k;
    sc->pbest = sc->best;
    sc->best = JAYA_INF;
    sc->fev += np;
    sc->gen = gen + 1;
    if (c.adapt) {
        double *perf = d.perfindex + (size_t) p * nks, *ps = d.pstrat + (size_t) p * nks;
        const double imp = (sc->pbest - sc->best) / (fabs(sc->pbest) > 1e-12 ? fabs(sc->pbest) : 1e-12);
        perf[k - 1] = imp;
        ps[k - 1] = exp(c.temper * imp);
        double total = 0.;
        for (int q = 0; q < nks; q++) total += ps[q];
        const u32x4 w = philox4x32_10_uniform(c.seed, JAYA_CTRL_ROULETTE, 0, (uint32_t) gen,
                stream_word(STREAM_JAYA_CTRL, (uint32_t) p));
        const double u = u01(w.x, w.y);
        double U = u * total;
        int next = nks;
        for (int q = 0; q < nks; q++) {
            U -= ps[q];
            if (U <= 0.) {
                next = q + 1;
                break;
            }
        }
        sc->k = next;
        sc->uroul = u;
    }
    // optimize(), jaya.cpp:184-196: the budget is looked at before the spread
    if (sc->fev >= c.mfev) sc->stop = 2;
    else if (conv) sc->stop = 1;
}

} // namespace bbo
