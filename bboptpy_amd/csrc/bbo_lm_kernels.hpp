// bbo_lm_kernels.hpp -- one LM-CMA-ES generation as gfx950 kernels (grid.y or .x = population).
//
//   kernel           reference lines (lm_cmaes.cpp)                            work per population
//   lm_draw          :94-106 z of the "+" candidates, :314 the subset normal    lambda n / 8 Philox calls
//   lm_sample        :108-124 the dots, the fold, both mirrored rows            lambda m n flops
//   lm_eval          :215-226 fp <- the last sorted values, the objective       lambda n
//   lm_rank          base_cmaes.cpp:221 (rank by counting)                      lambda^2 compares
//   lm_update        :129-181 mean, pc, updateSet, ainvz, b, d; :228-258 sigma  mu n + up to m^2 n
//   lm_history_stop  base :191-209, :183-213                                    hlen + n
//
// A dot product over n is added the same way everywhere: thread t of the 256 sums the terms t,
// t + 256, ... in order (its NR = ceil(n / 256) own columns, which it keeps in registers), a xor
// butterfly adds the 64 lanes of a wavefront and the four wavefronts are added from left to right
// (block_sum<4>; lm_sample parks the wavefronts' sums of all its dots in LDS and adds them behind one
// barrier).  tests/lm_model.py (dev_dot) states the same order.
#pragma once

#include "bbo_lm.hpp"
#include "bbo_objectives.hpp"
#include "bbo_rank.hpp"
#include "bbo_rng.hpp"
#include "bbo_wave.hpp"

namespace bbo {

#define LM_INF (__builtin_huge_val())

// z of the "+" candidates: a wavefront per row k, lane q takes the Philox call (k, q, generation,
// population) -- four ziggurat normals, or four coins (+1 where the word's top bit is clear: u < 0.5)
// -- for the columns 4 q .. 4 q + 3; lane 0 also draws the normal of selectSubset from a stream of
// its own (drawn always, used where the reference draws one).  grid (ceil(half / 4), P), 256 threads
__global__ __launch_bounds__(256) void lm_draw(LmDev d, LmConst c)
{
    const int p = blockIdx.y;
    const LmScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.x * 4 + wave, n = c.n;
    if (k >= c.half) return;
    const size_t row = (size_t) p * c.half + k;
    double *z = d.Z + row * c.ld;
    const uint32_t gen = (uint32_t) sc->it, sw = stream_word(STREAM_LM_Z, (uint32_t) p);
    const double2 *wk = zig_global_wk();
    for (int q = lane; 4 * q < n; q += 64) {
        double v[4];
        if (c.rademacher) {
            const u32x4 w = philox4x32_10(c.seed, (uint32_t) k, (uint32_t) q, gen, sw);
            v[0] = (w.x >> 31) ? -1. : 1.;
            v[1] = (w.y >> 31) ? -1. : 1.;
            v[2] = (w.z >> 31) ? -1. : 1.;
            v[3] = (w.w >> 31) ? -1. : 1.;
        } else {
            normal_quad(c.seed, (uint32_t) k, (uint32_t) q, gen, sw, wk, v[0], v[1], v[2], v[3]);
        }
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (4 * q + t < n) z[4 * q + t] = v[t];
    }
    if (lane == 0) {
        double g0, g1, g2, g3;
        normal_quad(c.seed, (uint32_t) k, 0u, gen, stream_word(STREAM_LM_SUBSET, (uint32_t) p), wk, g0, g1, g2, g3);
        d.g[row] = g0;
    }
}

// The candidates of LM_BLOCK "+" rows and their mirrors.  i0 of a row is selectSubset's (:304-318).
// The dot of slot i is taken with the original z (:117-119), so all of them are formed first: V
// streams in once for the block, a thread multiplies its columns of a row of V with its columns of
// the block's z, which it holds in registers.  Then the fold (:120-121) runs per column from the
// smallest i0 of the block on, P streaming in once, a row joining at its own i0, and x = m +- sigma az
// (:124) is written.  NR = ceil(n / 256).  grid (ceil(half / LM_BLOCK), P), 256 threads
template<int NR>
__global__ __launch_bounds__(256) void lm_sample(LmDev d, LmConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const LmScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    __shared__ double part[LM_MAX_M * LM_BLOCK * 4];
    __shared__ double dots[LM_MAX_M * LM_BLOCK];
    __shared__ int sj[LM_MAX_M];
    __shared__ int si0[LM_BLOCK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = c.n, ld = c.ld, m = c.m, lambda = c.lambda;
    const int k0 = blockIdx.x * LM_BLOCK;
    const int memlen = min(sc->memlen, m);
    const double sigma = sc->sigma;
    const double *V = d.Vm + (size_t) p * m * ld, *Pm = d.Pm + (size_t) p * m * ld;
    const double *xm = d.xmean + (size_t) p * ld;
    if (tid < LM_BLOCK) {
        const int k = k0 + tid;
        int i0 = 0;
        if (k < c.half && c.usenew && memlen > 1) {
            // int(msigma |g|) capped at memlen; taking the smaller value first keeps the cast in range
            const double ms = fmin((k == 0 ? 40. : 4.) * fabs(d.g[(size_t) p * c.half + k]), (double) memlen);
            i0 = memlen - (int) ms;
        }
        si0[tid] = k < c.half ? i0 : memlen;
    }
    for (int i = tid; i < memlen; i += 256) sj[i] = min(max(d.jarr[(size_t) p * m + i], 0), m - 1);
    __syncthreads();
    int imin = memlen;
#pragma unroll
    for (int q = 0; q < LM_BLOCK; q++) imin = min(imin, si0[q]);

    double z[LM_BLOCK][NR];
#pragma unroll
    for (int q = 0; q < LM_BLOCK; q++) {
        const int k = min(k0 + q, c.half - 1);
        const double *zr = d.Z + ((size_t) p * c.half + k) * ld;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int col = tid + 256 * r;
            z[q][r] = col < n ? zr[col] : 0.;
        }
    }
    for (int i = imin; i < memlen; i++) {
        const double *vrow = V + (size_t) sj[i] * ld;
        double acc[LM_BLOCK];
#pragma unroll
        for (int q = 0; q < LM_BLOCK; q++) acc[q] = 0.;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int col = tid + 256 * r;
            if (col < n) {
                const double v = vrow[col];
#pragma unroll
                for (int q = 0; q < LM_BLOCK; q++) acc[q] += v * z[q][r];
            }
        }
#pragma unroll
        for (int q = 0; q < LM_BLOCK; q++) {
            const double s = group_sum<64>(acc[q]);
            if (lane == 0) part[(i * LM_BLOCK + q) * 4 + wave] = s;
        }
    }
    __syncthreads();
    for (int idx = tid + imin * LM_BLOCK; idx < memlen * LM_BLOCK; idx += 256) {
        const double *pp = part + idx * 4;
        dots[idx] = d.b[(size_t) p * m + sj[idx / LM_BLOCK]] * (((pp[0] + pp[1]) + pp[2]) + pp[3]);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const int col = tid + 256 * r;
        if (col >= n) continue;
        double az[LM_BLOCK];
#pragma unroll
        for (int q = 0; q < LM_BLOCK; q++) az[q] = z[q][r];
        for (int i = imin; i < memlen; i++) {
            const double pv = Pm[(size_t) sj[i] * ld + col];
#pragma unroll
            for (int q = 0; q < LM_BLOCK; q++)
                if (i >= si0[q]) az[q] = c.sqrt1mc1 * az[q] + dots[i * LM_BLOCK + q] * pv;
        }
        const double mj = xm[col];
#pragma unroll
        for (int q = 0; q < LM_BLOCK; q++) {
            const int k = k0 + q;
            if (k >= c.half) continue;
            double *x0 = d.X + ((size_t) p * lambda + 2 * k) * ld;
            x0[col] = mj + sigma * az[q];
            if (2 * k + 1 < lambda) x0[ld + col] = mj + (-sigma) * az[q];
        }
    }
}

// fp <- the sorted values of the last generation (:218-222; the first workgroup of a population),
// then the objective on the rows, a wavefront per row; a host objective evaluates X itself.
// grid (ceil(lambda / 4), P), 256 threads
__global__ __launch_bounds__(256) void lm_eval(LmDev d, LmConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const LmScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lambda = c.lambda;
    const size_t pf = (size_t) p * lambda;
    if (blockIdx.x == 0 && sc->it > 0)
        for (int i = threadIdx.x; i < lambda; i += 256) d.fp[pf + i] = d.fsort[pf + i];
    const int r = blockIdx.x * 4 + wave;
    if (c.obj < 0 || r >= lambda) return;
    double f = eval_row_group<64>(c.obj, c.n, d.X + (pf + r) * c.ld, d.aux, lane);
    if (f != f) f = LM_INF;
    if (lane == 0) d.f[pf + r] = f;
}

// order[k] = the index of rank k, rank[i] = the rank of index i, fsort[k] = the value of rank k; ties
// to the lower index.  grid (ceil(lambda / 32), P), 256 threads = 32 candidates x 8 slices
__global__ __launch_bounds__(256) void lm_rank(LmDev d, LmConst c)
{
    const int p = blockIdx.y;
    const LmScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    __shared__ __attribute__((aligned(16))) double tile[RANK_TILE];
    const int tid = threadIdx.x, lambda = c.lambda;
    const int cand = blockIdx.x * 32 + (tid >> 3), slice = tid & 7;
    const size_t pf = (size_t) p * lambda;
    const int cnt = rank_by_counting(d.f + pf, lambda, cand, slice, tile);
    if (cand < lambda && slice == 0 && cnt < lambda) {
        d.order[pf + cnt] = cand;
        d.rank[pf + cand] = cnt;
        d.fsort[pf + cnt] = d.f[pf + cand];
    }
}

// the number of entries of the ascending v[0, cnt) that are < x (STRICT) or <= x
template<bool STRICT>
__device__ inline int lm_count_before(const double *v, int cnt, double x)
{
    int lo = 0, hi = cnt;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const bool before = STRICT ? v[mid] < x : v[mid] <= x;
        lo = before ? mid + 1 : lo;
        hi = before ? hi : mid;
    }
    return lo;
}

// updateSet (:274-302) on one lane; returns imin
__device__ inline int lm_update_set(int *jarr, int *larr, int m, int it_gen, int t, int nsteps)
{
    const int it = it_gen / t;
    int imin = 1;
    if (it < m) {
        jarr[it] = it;
    } else if (m > 1) {
        int iminval = larr[jarr[1]] - larr[jarr[0]];
        for (int i = 1; i < m - 1; i++) {
            const int val = larr[jarr[i + 1]] - larr[jarr[i]];
            if (val < iminval) {
                iminval = val;
                imin = i + 1;
            }
        }
        if (iminval >= nsteps) imin = 0;
        const int jtmp = jarr[imin];
        for (int i = imin; i < m - 1; i++) jarr[i] = jarr[i + 1];
        jarr[m - 1] = jtmp;
    }
    larr[jarr[min(it, m - 1)]] = it_gen;
    return imin == 1 ? 0 : imin;
}

// One workgroup per population, a thread per column (NR columns each).  The mean is the weighted sum
// over the mu best in rank order and pc follows (:132-147): the reference's operations in its order.
// Every t-th generation one lane runs updateSet, pc goes into the newest slot and the v vectors of the
// slots from imin on are recomputed by ainvz (:162-176): the running vector stays in registers, v_k
// streams in, each step costs one workgroup reduction; then b and d.  The sigma rule (:228-258): this
// and the last generation's values are both sorted, so the pooled rank of an element is its own place
// plus the number of elements of the other list in front of it, a binary search; a previous value
// precedes an equal current one.  The numerator is an exact integer.  grid (P), 256 threads
template<int NR>
__global__ __launch_bounds__(256) void lm_update(LmDev d, LmConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    LmScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    __shared__ double scratch[4];
    __shared__ double sd[LM_MAX_M];
    __shared__ int sj[LM_MAX_M];
    __shared__ int s_imin, s_memlen, s_acc;
    const int tid = threadIdx.x, n = c.n, ld = c.ld, lambda = c.lambda, mu = c.mu, m = c.m;
    const size_t pv = (size_t) p * ld, pf = (size_t) p * lambda, pm = (size_t) p * m;
    const double sigma = sc->sigma;
    const int it = sc->it;
    const double *X = d.X + pf * ld;
    const int *order = d.order + pf;
    double *Pm = d.Pm + pm * ld, *Vm = d.Vm + pm * ld;

    double a[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const int col = tid + 256 * r;
        a[r] = 0.;
        if (col >= n) continue;
        const double xo = d.xmean[pv + col];
        double xm = 0.;
        for (int k = 0; k < mu; k++) xm = xm + d.w[k] * X[(size_t) min(max(order[k], 0), lambda - 1) * ld + col];
        if (c.bound) {
            // std::max(lower, std::min(xm, upper))
            const double lo = d.lower[col], up = d.upper[col];
            const double tmin = up < xm ? up : xm;
            xm = lo < tmin ? tmin : lo;
        }
        d.xold[pv + col] = xo;
        d.xmean[pv + col] = xm;
        const double pcv = (1. - c.cc) * d.pc[pv + col] + (c.ccc * (xm - xo)) / sigma;
        d.pc[pv + col] = pcv;
        a[r] = pcv;
    }

    if (it % c.t == 0) {
        if (tid == 0) {
            s_imin = lm_update_set(d.jarr + pm, d.larr + pm, m, it, c.t, c.nsteps);
            s_memlen = min(sc->memlen + 1, m);
        }
        __syncthreads();
        const int imin = s_imin, memlen = s_memlen;
        for (int i = tid; i < m; i += 256) {
            sj[i] = min(max(d.jarr[pm + i], 0), m - 1);
            sd[i] = d.d[pm + i];
        }
        __syncthreads();
        {
            double *prow = Pm + (size_t) sj[memlen - 1] * ld;
#pragma unroll
            for (int r = 0; r < NR; r++) {
                const int col = tid + 256 * r;
                if (col < n) prow[col] = a[r];
            }
        }
        const double cinv = 1. / c.sqrt1mc1;
        for (int i = imin; i < memlen; i++) {
            const int jcur = sj[i];
            // (the newest slot's row was written by this thread just now: the same columns)
#pragma unroll
            for (int r = 0; r < NR; r++) {
                const int col = tid + 256 * r;
                a[r] = col < n ? Pm[(size_t) jcur * ld + col] : 0.;
            }
            for (int k = 0; k < i; k++) {
                const int idx = sj[k];
                const double *vrow = Vm + (size_t) idx * ld;
                double vk[NR], part = 0.;
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    const int col = tid + 256 * r;
                    vk[r] = col < n ? vrow[col] : 0.;
                    if (col < n) part += vk[r] * a[r];
                }
                const double dot = sd[idx] * block_sum<4>(part, scratch);
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    a[r] = cinv * a[r];
                    a[r] = a[r] + (-dot) * vk[r];
                }
            }
            double part = 0.;
#pragma unroll
            for (int r = 0; r < NR; r++) {
                const int col = tid + 256 * r;
                if (col < n) {
                    Vm[(size_t) jcur * ld + col] = a[r];
                    part += a[r] * a[r];
                }
            }
            const double vnrm2 = block_sum<4>(part, scratch);
            const double sqrtc1 = sqrt(1. + (c.c1 / (1. - c.c1)) * vnrm2);
            const double dv = (1. / (c.sqrt1mc1 * vnrm2)) * (1. - 1. / sqrtc1);
            if (tid == 0) {
                d.b[pm + jcur] = (c.sqrt1mc1 / vnrm2) * (sqrtc1 - 1.);
                d.d[pm + jcur] = dv;
                sd[jcur] = dv;
            }
            __syncthreads();
        }
        if (tid == 0) sc->memlen = memlen;
    }

    if (it == 0) return;
    if (tid == 0) s_acc = 0;
    __syncthreads();
    const double *fs = d.fsort + pf, *fp = d.fp + pf;
    int mine = 0;
    for (int e = tid; e < 2 * lambda; e += 256) {
        if (e < lambda) mine += e + lm_count_before<true>(fs, lambda, fp[e]);
        else mine -= (e - lambda) + lm_count_before<false>(fp, lambda, fs[e - lambda]);
    }
    if (mine) atomicAdd(&s_acc, mine);
    __syncthreads();
    if (tid != 0) return;
    const double zpsr = (double) s_acc / ((double) lambda * (double) lambda) - c.zstar;
    const double s = (1. - c.cs) * sc->s + c.cs * zpsr;
    sc->s = s;
    sc->sigma = sigma * exp(s / c.damps);
}

// The histories of the best and the ik-th value and their extremes (base_cmaes.cpp:191-209), it++,
// fev += lambda, the four stop tests in the reference's order (:183-213) and the stop flag.
// grid (P), 64 threads
__global__ __launch_bounds__(64) void lm_history_stop(LmDev d, LmConst c)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    LmScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int n = c.n, hlen = c.hlen;
    double *hb = d.hist_best + (size_t) p * hlen, *hk = d.hist_kth + (size_t) p * hlen;
    const double *fs = d.fsort + (size_t) p * c.lambda;
    int it = sc->it, head = sc->hist_head, len = sc->hist_len;
    double fbest = sc->fbest, fworst = sc->fworst;
    if (it < c.mit) {
        head = (head + 1) % hlen;
        if (lane == 0) {
            hb[head] = fs[0];
            hk[head] = fs[c.ik];
        }
        if (len < hlen) len++;
        wave_sync();
        if (len == hlen) {
            double lo = LM_INF, hi = -LM_INF;
            for (int k = lane; k < hlen; k += 64) {
                lo = fmin(lo, hb[k]);
                hi = fmax(hi, hb[k]);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                lo = fmin(lo, __shfl_xor(lo, off, 64));
                hi = fmax(hi, __shfl_xor(hi, off, 64));
            }
            fbest = lo;
            fworst = hi;
        }
    }
    it++;
    wave_sync();
    int flag = 0;
    if (it >= c.mit) {
        flag = 1;
    } else if (sc->sigma < c.stolmin) {
        flag = LM_FLAG_SIGMA;
    } else if (it >= hlen && fworst - fbest < c.tol) {
        flag = 2;
    } else if (len >= n) {
        int eq = 0;
        for (int i = lane; i < n; i += 64) {
            const int idx = (hlen + head - i) % hlen;
            eq += hb[idx] == hk[idx];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) eq += __shfl_xor(eq, off, 64);
        if (3 * eq >= n) flag = 3;
    }
    if (lane == 0) {
        const int fev = sc->fev + c.lambda;
        sc->it = it;
        sc->fev = fev;
        sc->hist_head = head;
        sc->hist_len = len;
        sc->fbest = fbest;
        sc->fworst = fworst;
        sc->flag = flag;
        sc->conv = flag ? 1 : 0;
        if (flag) sc->stop = 1;
        else if (fev >= c.mfev) sc->stop = 2;
    }
}

} // namespace bbo
