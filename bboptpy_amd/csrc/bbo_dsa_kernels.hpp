// bbo_dsa_kernels.hpp -- one DSA generation as gfx950 kernels.
//
//   kernel        reference lines (ds.cpp)                                bytes per member
//   dsa_init      :294-302 uniform pool, its fitness                      8n written
//   dsa_rank      the std::sort of :245-248 / :266-269 (rank by counting;  8 (returns at once under
//                 ties to the lower row)                                   methods 1 and 4)
//   dsa_plan      :91-116 p1, p2, method, R; :307-333 the map strategy;    4
//                 :219-292 the direction row of every member
//   dsa_evolve    :119-137 trial, :344-365 box repair, evaluation,         8n own row + 8n direction
//                 selection into the other half of the double buffer       row read, 8n written: 24n,
//                                                                          against one Philox call per
//                                                                          coordinate
//   dsa_select    :132-136 for a host objective (the trials come back with their f)
//   dsa_finish    :138-155 successes and the bandit, :186-217 the stop test  20
#pragma once

#include "bbo_dsa.hpp"
#include "bbo_objectives.hpp"
#include "bbo_rank.hpp"
#include "bbo_rng.hpp"

namespace bbo {

#define DSA_INF (__builtin_huge_val())

// what a draw of the control stream is for (counter word 0)
enum { DSA_CTRL_P = 0, DSA_CTRL_METHOD = 1, DSA_CTRL_MAP = 2 };
enum { DSA_MAP_RANDOM1 = 0, DSA_MAP_DIFFERENTIAL = 1, DSA_MAP_RANDOM2 = 2 };

// The method index of this generation (ds.cpp:94-101) and the two uniforms of its Philox call.
// `adapt`: std::discrete_distribution over p -- probabilities p[i] / sum, their running sums, the
// first one above u (the last counts as 1).  Else uniform in 0..3.  A function of (generation,
// population, p) alone: dsa_rank and dsa_plan both call it and agree.
__device__ inline int dsa_method(const DsaConst &c, const DsaScal *sc, int p, double &u, double &ucoin)
{
    const u32x4 w = philox4x32_10_uniform(c.seed, DSA_CTRL_METHOD, 0, (uint32_t) sc->gen,
            stream_word(STREAM_DSA_CTRL, (uint32_t) p));
    u = u01(w.x, w.y);
    ucoin = u01(w.z, w.w);
    int m;
    if (c.adapt) {
        const double sum = ((sc->p[0] + sc->p[1]) + sc->p[2]) + sc->p[3];
        const double c0 = sc->p[0] / sum, c1 = c0 + sc->p[1] / sum, c2 = c1 + sc->p[2] / sum;
        m = u < c0 ? 0 : u < c1 ? 1 : u < c2 ? 2 : 3;
    } else {
        m = (int) (u * 4.);
    }
    return c.force_method >= 0 ? c.force_method : m;
}

// genPop, ds.cpp:294-302: a wavefront per member.  grid (ceil(np / 4), P), 256 threads, LDS
// 4 * ld doubles
__global__ __launch_bounds__(256) void dsa_init(DsaDev d, DsaConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave, n = c.n, ld = c.ld;
    if (i >= c.np) return;
    const size_t pb = (size_t) p * c.np;
    double *x = d.X[0] + (pb + i) * ld, *row = lds + wave * ld;
    double ssq = 0.;
    for (int j = lane; j < n; j += 64) {
        const u32x4 w = philox4x32_10(c.seed, (uint32_t) i, (uint32_t) j, 0,
                stream_word(STREAM_INIT, (uint32_t) p));
        const double v = u01(w.x, w.y) * (d.upper[j] - d.lower[j]) + d.lower[j];
        x[j] = v;
        row[j] = v;
        ssq += v * v;
    }
    wave_sync();
    ssq = group_sum<64>(ssq);
    double f = DSA_INF;
    if (c.obj >= 0) {
        f = eval_row_group<64>(c.obj, n, row, d.aux, lane);
        if (f != f) f = DSA_INF;
    }
    if (lane == 0) {
        d.f[pb + i] = f;
        d.radius[pb + i] = sqrt(ssq);
    }
}

// order[r] = the row of rank r by f, ties to the lower row.  Launched every generation; under the
// methods that do not sort (1 and 4) every workgroup leaves on a uniform branch.
// grid (ceil(np / 32), P), 256 threads = 32 rows x 8 slices
__global__ __launch_bounds__(256) void dsa_rank(DsaDev d, DsaConst c)
{
    const int p = blockIdx.y;
    const DsaScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    double u, ucoin;
    const int m = dsa_method(c, sc, p, u, ucoin);
    if (m != 1 && m != 2) return;
    __shared__ __attribute__((aligned(16))) double tile[RANK_TILE];
    const int tid = threadIdx.x, np = c.np;
    const int cand = blockIdx.x * 32 + (tid >> 3), slice = tid & 7;
    const size_t pb = (size_t) p * np;
    const int cnt = rank_by_counting(d.f + pb, np, cand, slice, tile);
    if (cand < np && slice == 0) d.order[pb + cnt] = cand;
}

// The generation's scalars and the direction row of every member.  One workgroup per population.
// grid (P), 256 threads
__global__ __launch_bounds__(256) void dsa_plan(DsaDev d, DsaConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    DsaScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    __shared__ int s_method;
    __shared__ double smin[4];
    __shared__ int srow[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, np = c.np, n = c.n;
    const uint32_t gen = (uint32_t) sc->gen;
    const size_t pb = (size_t) p * np;
    if (tid == 0) {
        const uint32_t ctrl = stream_word(STREAM_DSA_CTRL, (uint32_t) p);
        const u32x4 w0 = philox4x32_10_uniform(c.seed, DSA_CTRL_P, 0, gen, ctrl);
        const u32x4 w2 = philox4x32_10_uniform(c.seed, DSA_CTRL_MAP, 0, gen, ctrl);
        const double up1 = u01(w0.x, w0.y), up2 = u01(w0.z, w0.w);
        const double ustrat = u01(w2.x, w2.y), ur = u01_open0(w2.z, w2.w);
        double um, ucoin;
        const int method = dsa_method(c, sc, p, um, ucoin);
        const double p1 = up1 * 0.3, p2 = up2 * 0.3;              // Random::get(0.0, 0.3)
        // genMap, ds.cpp:307-333: the coin, then `u < p1`
        int strategy = ucoin < 0.5 ? (ustrat < p1 ? DSA_MAP_RANDOM1 : DSA_MAP_DIFFERENTIAL) : DSA_MAP_RANDOM2;
        if (c.force_map >= 0) strategy = c.force_map;
        // :116; u = 1 would divide by -0: R = 0, what the reference's u = 0 gives
        const double R = ur == 1. ? 0. : 1. / (-2. * log_unit(ur));
        sc->raw[0] = up1;
        sc->raw[1] = up2;
        sc->raw[2] = um;
        sc->raw[3] = ucoin;
        sc->raw[4] = ustrat;
        sc->raw[5] = ur;
        sc->p1 = p1;
        sc->p2 = p2;
        sc->R = R;
        sc->method = method;
        sc->strategy = strategy;
        sc->mapmax = (int) ceil(p2 * n);
        s_method = method;
    }
    __syncthreads();
    const int method = s_method;
    int *dirrow = d.dirrow + pb;
    const int *order = d.order + pb;
    double *dd = d.dirdraws ? d.dirdraws + pb * 2 : nullptr;
    if (method == 0) {
        // B-DSA, :226-234: std::shuffle of the rows -> the keyed bijection
        for (int i = tid; i < np; i += 256) {
            const int r = (int) cso_perm((uint32_t) i, c.kb, (uint32_t) np, c.seed, gen,
                    stream_word(STREAM_DSA_PERM, (uint32_t) p));
            dirrow[i] = r;
            if (dd) {
                dd[2 * i] = r;
                dd[2 * i + 1] = 0.;
            }
        }
    } else if (method == 1) {
        // S-DSA, :249-255: one of the ub best, ub = ceil(u np) drawn per member (u = 0: the
        // reference indexes out of its array; here ub = 1)
        for (int i = tid; i < np; i += 256) {
            const u32x4 w = philox4x32_10(c.seed, (uint32_t) i, 0, gen, stream_word(STREAM_DSA_DIR, (uint32_t) p));
            const double u = u01(w.x, w.y);
            const int ub = min(max((int) ceil(u * np), 1), np);
            dirrow[i] = order[uint_below(w.z, ub)];
            if (dd) {
                dd[2 * i] = u;
                dd[2 * i + 1] = (double) w.z;
            }
        }
    } else if (method == 2) {
        // E1-DSA, :270-275: rank min(ub, np - 1), once for all members
        const u32x4 w = philox4x32_10_uniform(c.seed, 0, 1, gen, stream_word(STREAM_DSA_DIR, (uint32_t) p));
        const double u = u01(w.x, w.y);
        const int r = order[min((int) ceil(u * np), np - 1)];
        for (int i = tid; i < np; i += 256) {
            dirrow[i] = r;
            if (dd) {
                dd[2 * i] = i == 0 ? u : 0.;
                dd[2 * i + 1] = 0.;
            }
        }
    } else {
        // E2-DSA, :283-288: the first minimum in row order
        double fmin = DSA_INF;
        int rmin = 0x7fffffff;
        for (int i = tid; i < np; i += 256) {
            const double fv = d.f[pb + i];
            if (fv < fmin || (fv == fmin && i < rmin)) {
                fmin = fv;
                rmin = i;
            }
        }
        wave_argmin(fmin, rmin);
        if (lane == 0) {
            smin[wave] = fmin;
            srow[wave] = rmin;
        }
        __syncthreads();
        fmin = smin[0];
        rmin = srow[0];
        for (int w = 1; w < 4; w++)
            if (smin[w] < fmin || (smin[w] == fmin && srow[w] < rmin)) {
                fmin = smin[w];
                rmin = srow[w];
            }
        rmin = min(rmin, np - 1);
        for (int i = tid; i < np; i += 256) {
            dirrow[i] = rmin;
            if (dd) dd[2 * i] = dd[2 * i + 1] = 0.;
        }
    }
}

// A wavefront per member: lanes stride the coordinates.  The Philox call (row, j, generation)
// supplies coordinate j's map uniform (words 0, 1), its boundary uniform (words 2, 3) and its
// boundary coin (bit 0 of word 2, which the uniform does not use); the call (row, 0, generation) of
// the map stream the member's `rand` (random-1) and its one coordinate (differential); the calls
// (row, 1 + q, generation) the coordinates 4q .. 4q + 3 of random-2, which the lanes mark in LDS.
// The trial is formed in the reference's operation order.  The direction row is another member's
// row as it stood at the start of the generation: the pool is read from X[cur] and the member's
// next row -- the trial if it wins, else its old row -- is written to X[cur ^ 1].
// grid (ceil(np / 4), P), 256 threads, LDS 4 * ld doubles
__global__ __launch_bounds__(256) void dsa_evolve(DsaDev d, DsaConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const DsaScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave, n = c.n, ld = c.ld;
    if (i >= c.np) return;
    const uint32_t gen = (uint32_t) sc->gen;
    const int cur = sc->cur, strategy = sc->strategy, mapmax = min(sc->mapmax, c.mcap);
    const double R = sc->R;
    const size_t pb = (size_t) p * c.np;
    const int drow = min(max(d.dirrow[pb + i], 0), c.np - 1);
    const double *x = d.X[cur] + (pb + i) * ld;
    const double *dir = d.X[cur] + (pb + drow) * ld;
    double *xn = d.X[cur ^ 1] + (pb + i) * ld;
    double *tg = d.T ? d.T + (pb + i) * ld : nullptr;
    double *md = d.mapdraws ? d.mapdraws + (pb + i) * (n + 2 + c.mcap) : nullptr;
    double *bd = d.mapdraws ? d.bounddraws + (pb + i) * n * 2 : nullptr;
    int *mp = d.mapdraws ? d.map + (pb + i) * n : nullptr;
    double *trial = lds + wave * ld;
    const uint32_t swm = stream_word(STREAM_DSA_MAP, (uint32_t) p);
    const uint32_t swr = stream_word(STREAM_DSA_R, (uint32_t) p);
    const u32x4 wm = philox4x32_10(c.seed, (uint32_t) i, 0, gen, swm);
    const double rnd = u01(wm.x, wm.y);
    const int jd = uint_below(wm.z, n);
    if (md && lane == 0) {
        md[n] = rnd;
        md[n + 1] = (double) wm.z;
    }
    if (strategy == DSA_MAP_RANDOM2) {
        for (int j = lane; j < n; j += 64) trial[j] = 0.;
        wave_sync();
        for (int q = lane; 4 * q < mapmax; q += 64) {
            const u32x4 w = philox4x32_10(c.seed, (uint32_t) i, (uint32_t) (1 + q), gen, swm);
            const uint32_t ws[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int k = 4 * q + t;
                if (k < mapmax) {
                    trial[uint_below(ws[t], n)] = 1.;
                    if (md) md[n + 2 + k] = (double) ws[t];
                }
            }
        }
        wave_sync();
    }
    double ssq = 0.;
    for (int j = lane; j < n; j += 64) {
        const u32x4 w = philox4x32_10(c.seed, (uint32_t) i, (uint32_t) j, gen, swr);
        const double um = u01(w.x, w.y), ub = u01(w.z, w.w);
        const int coin = (int) (w.z & 1u);
        const int m = strategy == DSA_MAP_RANDOM1 ? (um < rnd ? 1 : 0)
                : strategy == DSA_MAP_DIFFERENTIAL ? (j == jd ? 1 : 0) : (trial[j] != 0. ? 1 : 0);
        const double xj = x[j], dj = dir[j], lo = d.lower[j], up = d.upper[j];
        double t = xj + (R * (double) m) * (dj - xj);
        // update(), ds.cpp:344-365
        if (t < lo) t = coin == 0 ? ub * (up - lo) + lo : lo;
        if (t > up) t = coin == 0 ? ub * (up - lo) + lo : up;
        trial[j] = t;
        if (tg) tg[j] = t;
        if (md) {
            md[j] = um;
            bd[2 * j] = coin;
            bd[2 * j + 1] = ub;
            mp[j] = m;
        }
        ssq += t * t;
    }
    if (c.obj < 0) return;      // a host objective: dsa_select finishes the member
    wave_sync();
    ssq = group_sum<64>(ssq);
    double ft = eval_row_group<64>(c.obj, n, trial, d.aux, lane);
    if (ft != ft) ft = DSA_INF;
    const bool take = ft < d.f[pb + i];
    for (int j = lane; j < n; j += 64) xn[j] = take ? trial[j] : x[j];
    if (lane == 0) {
        d.ftrial[pb + i] = ft;
        d.acc[pb + i] = take ? 1 : 0;
        if (take) {
            d.f[pb + i] = ft;
            d.radius[pb + i] = sqrt(ssq);
        }
    }
}

// greedy selection from T / ftrial into X[cur ^ 1] (host objective).
// grid (ceil(np / 4), P), 256 threads
__global__ __launch_bounds__(256) void dsa_select(DsaDev d, DsaConst c)
{
    const int p = blockIdx.y;
    const DsaScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave, n = c.n, ld = c.ld, cur = sc->cur;
    if (i >= c.np) return;
    const size_t pb = (size_t) p * c.np;
    const double ft = d.ftrial[pb + i];
    const bool take = ft < d.f[pb + i];
    const double *src = (take ? d.T : d.X[cur]) + (pb + i) * ld;
    double *xn = d.X[cur ^ 1] + (pb + i) * ld;
    double ssq = 0.;
    for (int j = lane; j < n; j += 64) {
        const double v = src[j];
        xn[j] = v;
        ssq += v * v;
    }
    ssq = group_sum<64>(ssq);
    if (lane == 0) {
        d.acc[pb + i] = take ? 1 : 0;
        if (take) {
            d.f[pb + i] = ft;
            d.radius[pb + i] = sqrt(ssq);
        }
    }
}

// The successes, the Rexp3 update of w and p (ds.cpp:141-154), it++, fev += np, converged()
// (:186-217: |fmin - fmax| <= tol and then the spread of the radii; the radii are plain root sums
// of squares and their spread a two-pass sum), the incumbent (the first
// minimum in row order) and the flip of the double buffer.  grid (P), 256 threads
__global__ __launch_bounds__(256) void dsa_finish(DsaDev d, DsaConst c, int init_only)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    DsaScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    __shared__ double smin[4], smax[4], ssum[4];
    __shared__ int srow[4], scnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, np = c.np;
    const size_t pb = (size_t) p * np;
    const int now = init_only ? sc->cur : sc->cur ^ 1;      // the half that holds the pool now
    double fmin = DSA_INF, fmax = -DSA_INF, rsum = 0.;
    int rmin = 0x7fffffff, cnt = 0;
    for (int i = tid; i < np; i += 256) {
        const double fv = d.f[pb + i];
        if (fv < fmin || (fv == fmin && i < rmin)) {
            fmin = fv;
            rmin = i;
        }
        fmax = fv > fmax ? fv : fmax;
        rsum += d.radius[pb + i];
        if (!init_only) cnt += d.acc[pb + i];
    }
    wave_argmin(fmin, rmin);
    rsum = group_sum<64>(rsum);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(fmax, off, 64);
        fmax = ov > fmax ? ov : fmax;
        cnt += __shfl_xor(cnt, off, 64);
    }
    if (lane == 0) {
        smin[wave] = fmin;
        srow[wave] = rmin;
        smax[wave] = fmax;
        ssum[wave] = rsum;
        scnt[wave] = cnt;
    }
    __syncthreads();
    fmin = smin[0];
    rmin = srow[0];
    fmax = smax[0];
    for (int w = 1; w < 4; w++) {
        if (smin[w] < fmin || (smin[w] == fmin && srow[w] < rmin)) {
            fmin = smin[w];
            rmin = srow[w];
        }
        fmax = smax[w] > fmax ? smax[w] : fmax;
    }
    rmin = min(rmin, np - 1);
    const int nsucc = (scnt[0] + scnt[1]) + (scnt[2] + scnt[3]);
    const double mean = ((ssum[0] + ssum[1]) + (ssum[2] + ssum[3])) / np;
    double m2 = 0.;
    for (int i = tid; i < np; i += 256) {
        const double dd = d.radius[pb + i] - mean;
        m2 += dd * dd;
    }
    m2 = group_sum<64>(m2);
    __syncthreads();
    if (lane == 0) ssum[wave] = m2;
    __syncthreads();
    m2 = (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]);
    for (int j = tid; j < c.ld; j += 256)
        d.bestx[(size_t) p * c.ld + j] = d.X[now][(pb + rmin) * c.ld + j];
    if (tid != 0) return;
    sc->fbest = fmin;
    sc->m2 = m2;
    const int conv = fabs(fmin - fmax) <= c.tol && m2 <= (np - 1) * c.stol * c.stol ? 1 : 0;
    sc->conv = conv;
    if (init_only) return;
    sc->nsucc = nsucc;
    sc->fev += np;
    if (c.adapt) {
        const int im = sc->method;
        if (sc->it % c.nbatch == 0)
            for (int q = 0; q < 4; q++) sc->w[q] = 1.;
        const double reward = (1. * nsucc) / np;
        sc->w[im] *= exp(c.gamma * (reward / sc->p[im]) / 4);
        double wsum = 0.;
        for (int q = 0; q < 4; q++) wsum += sc->w[q];
        for (int q = 0; q < 4; q++) sc->p[q] = (1. - c.gamma) * sc->w[q] / wsum + c.gamma / 4;
    }
    sc->it++;
    sc->gen++;
    sc->cur = now;
    // optimize(), ds.cpp:172-178: converged() ends the loop, else its head looks at the budget
    if (conv) sc->stop = 1;
    else if (sc->fev >= c.mfev) sc->stop = 2;
}

} // namespace bbo
