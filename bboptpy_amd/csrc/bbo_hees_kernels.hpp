// bbo_hees_kernels.hpp -- one HEES generation as gfx950 kernels (grid.y or .z = population).
//
//   kernel        reference lines (hees.cpp)                              work per population
//   hees_draw     :203-209 the normals of rows r < mu, their norms         mu n / 4 Philox calls
//                 (hees_settle: the draws the fast test left open, the norms;
//                 hees_take: the same rows from an injected table)
//   hees_ortho    :211-229 modified Gram-Schmidt per batch, the rescale    2 mu min(mu, n) n flops
//   hees_points   :231-249 Y = b A^T, x = m -+ sigma y, the objective      2 mu n^2 flops
//                 (hees_points_mfma from half a tile of rows on)
//   hees_rank     :251-259 (rank by counting; ties to the lower index)     (2 mu)^2 compares
//   hees_update   :262-292, :324-364 h, q, m, p_s, g_s, sigma              4 mu n flops
//   hees_adapt    :294-321 as the low-rank update of bbo_hees.hpp          2 mu n^2 flops
//                 (hees_adapt_mfma likewise)
//   hees_finish   :332-340 f(m), the incumbent; :366-382 the stop test     n + 4 mu
#pragma once

#include "bbo_hees.hpp"
#include "bbo_objectives.hpp"
#include "bbo_rank.hpp"
#include "bbo_rng.hpp"
#include "bbo_wave.hpp"

namespace bbo {

#define HEES_INF (__builtin_huge_val())

// v_mfma_f64_16x16x4_f64 as bbo_cma_kernels.hpp uses it: A fragment = one double per lane,
// A[row = lane & 15][k = lane >> 4]; B fragment B[k = lane >> 4][col = lane & 15]; C/D = 4 doubles
// per lane, col = lane & 15, row = (lane >> 4) + 4 * reg.  (That header defines its kernels and
// cannot be included twice in one library: the vector type is repeated here.)
typedef double hees_d4 __attribute__((ext_vector_type(4)));

// Rows r < mu of Z: a wavefront per row, lane q takes the Philox call (row, q, generation,
// population) -- four ziggurat normals, one per word, columns 4 q .. 4 q + 3.  The rows above mu
// that the reference draws are never used and are not drawn.  Two kernels, so that neither holds
// more scalar state than the register file has: hees_draw forms the fast-path candidate of every
// word (99.57 % stand) and leaves a NaN where the fast test did not settle the draw; hees_settle
// finds those, recomputes their word, takes the slow path, and forms the row's norm.  The slow
// path holds some thirty fp64 constants and the Philox key schedule; with the seed in a scalar
// register the schedule is scalar too and sixteen scalar registers spilled into vector lanes, so
// hees_settle reads the seed per lane (lane_seed: the same value 64 times) and the schedule is
// computed in vector registers, of which the kernel has plenty.
// grid (ceil(mu / 4), P), 256 threads, both
__global__ __launch_bounds__(256) void hees_draw(HeesDev d, HeesConst c)
{
    const int p = blockIdx.y;
    const HeesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave, n = c.n;
    if (r >= c.mu) return;
    double *z = d.b + ((size_t) p * c.mu + r) * c.ld;
    const uint32_t gen = (uint32_t) sc->gen, sw = stream_word(STREAM_HEES_NORMAL, (uint32_t) p);
    const double2 *wk = zig_global_wk();
    for (int q = lane; 4 * q < n; q += 64) {
        const u32x4 w = philox4x32_10(c.seed, (uint32_t) r, (uint32_t) q, gen, sw);
        const uint32_t ws[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
        for (int t = 0; t < 4; t++) {
            bool settled;
            const double v = zig_candidate(ws[t], wk[ws[t] & 1023u], settled);
            if (4 * q + t < n) z[4 * q + t] = settled ? v : __builtin_nan("");
        }
    }
}

__global__ __launch_bounds__(256) void hees_settle(HeesDev d, HeesConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const HeesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave, n = c.n;
    if (r >= c.mu) return;
    const size_t row = (size_t) p * c.mu + r;
    double *z = d.b + row * c.ld;
    double *zl = d.zlast ? d.zlast + row * c.ld : nullptr;
    const uint32_t gen = (uint32_t) sc->gen, sw = stream_word(STREAM_HEES_NORMAL, (uint32_t) p);
    const uint64_t seed = d.lane_seed[lane];
    double ssq = 0.;
    for (int j = lane; j < n; j += 64) {
        double v = z[j];
        if (v != v) {
            const uint32_t q = (uint32_t) j >> 2, slot = (uint32_t) j & 3u;
            const u32x4 w4 = philox4x32_10(seed, (uint32_t) r, q, gen, sw);
            const uint32_t lo = (slot & 1u) ? w4.y : w4.x, hi = (slot & 1u) ? w4.w : w4.z;
            const uint32_t w = (slot & 2u) ? hi : lo;
            [[clang::always_inline]] v = zig_slow(seed, (uint32_t) r, q, slot, gen, sw, w & 1023u, (w >> 10) | 1u, (w >> 10) & 1u,
                    zig_global_wk(), zig_global_f());
            z[j] = v;
        }
        if (zl) zl[j] = v;
        ssq += v * v;
    }
    ssq = group_sum<64>(ssq);
    if (lane == 0) d.norms[row] = sqrt(ssq);
}

// A = I (the buffer arrives zeroed).  grid (P), 256 threads
__global__ __launch_bounds__(256) void hees_eye(HeesDev d, HeesConst c)
{
    double *A = d.A + (size_t) blockIdx.x * c.n * c.ld;
    for (int i = threadIdx.x; i < c.n; i += 256) A[(size_t) i * c.ld + i] = 1.;
}

// The same rows from the caller's table (injection) instead of the generator.
// grid (ceil(mu / 4), P), 256 threads
__global__ __launch_bounds__(256) void hees_take(HeesDev d, HeesConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const HeesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave, n = c.n;
    if (r >= c.mu) return;
    const size_t row = (size_t) p * c.mu + r;
    const double *zi = d.zin + row * c.ld;
    double *z = d.b + row * c.ld;
    double *zl = d.zlast ? d.zlast + row * c.ld : nullptr;
    double ssq = 0.;
    for (int j = lane; j < n; j += 64) {
        const double v = zi[j];
        z[j] = v;
        if (zl) zl[j] = v;
        ssq += v * v;
    }
    ssq = group_sum<64>(ssq);
    if (lane == 0) d.norms[row] = sqrt(ssq);
}

// Right-looking modified Gram-Schmidt over the live rows of one batch: one workgroup per (batch,
// population).  At step k every wavefront takes the norm of row k (finished: nobody writes it any
// more) and the later rows i, each owned by wavefront i mod W (W = 4, or 16 for a batch of 64 rows
// and more: the rows are independent chains of latency), do v_i -= (v^_k . v_i) v^_k with
// v^_k = v_k / |v_k|.  For every row that is the sequence of operations of the reference's
// left-looking loop (:213-223); a dot product is a wavefront reduction.  One barrier per step
// publishes the rows the step changed.  The rows stay unnormalised where they lie (1 / |v_k| is kept
// in LDS), the last pass writes (v_k / |v_k|) |z_k| (:222, :227-229).  use_lds: the rows are staged
// in LDS; else they are worked on where they are in global memory -- the same code and the same
// operation order.  grid (B, P), 256 or 1024 threads, LDS rows * ld doubles or none
__global__ __launch_bounds__(1024) void hees_ortho(HeesDev d, HeesConst c, int use_lds)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y, jb = blockIdx.x;
    const HeesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    extern __shared__ double lds[];
    __shared__ double sinv[HEES_MAX_N];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = c.n, ld = c.ld;
    const int nt = blockDim.x, nw = nt >> 6;
    const int row0 = jb * n, rows = min(n, c.mu - row0);
    if (rows <= 0) return;
    const size_t base = (size_t) p * c.mu + row0;
    double *g = d.b + base * ld;
    double *v = use_lds ? lds : g;
    if (use_lds)
        for (int idx = tid; idx < rows * ld; idx += nt) lds[idx] = g[idx];
    __syncthreads();
    for (int k = 0; k < rows; k++) {
        const double *vk = v + (size_t) k * ld;
        double s = 0.;
        for (int j = lane; j < n; j += 64) s += vk[j] * vk[j];
        s = group_sum<64>(s);
        const double inv = 1. / sqrt(s);
        if (tid == 0) sinv[k] = inv;
        for (int i = k + 1 + ((wave - (k + 1)) & (nw - 1)); i < rows; i += nw) {
            double *vi = v + (size_t) i * ld;
            double dt = 0.;
            for (int j = lane; j < n; j += 64) dt += (vk[j] * inv) * vi[j];
            dt = group_sum<64>(dt);
            for (int j = lane; j < n; j += 64) vi[j] = vi[j] + (-dt) * (vk[j] * inv);
        }
        __syncthreads();
    }
    for (int i = wave; i < rows; i += nw) {
        const double inv = sinv[i], nz = d.norms[base + i];
        for (int j = lane; j < n; j += 64) g[(size_t) i * ld + j] = (v[(size_t) i * ld + j] * inv) * nz;
    }
}

// Y = b A^T and the mirrored candidates: a wavefront per row r < mu.  The row b_r waits in LDS, lane
// i forms y_i = A_i . b_r in the reference's order (:234-235), x_r = m - sigma y and x_{r + mu} =
// m + sigma y go to LDS and the objective is evaluated on them there.  Y is kept; X leaves the LDS
// only for a host objective.  grid (ceil(mu / 4), P), 256 threads, LDS 12 ld doubles
__global__ __launch_bounds__(256) void hees_points(HeesDev d, HeesConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const HeesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave, n = c.n, ld = c.ld, mu = c.mu;
    if (r >= mu) return;
    const size_t row = (size_t) p * mu + r;
    double *bl = lds + (size_t) wave * 3 * ld, *xm = bl + ld, *xp = xm + ld;
    const double *br = d.b + row * ld, *A = d.A + (size_t) p * n * ld, *m = d.m + (size_t) p * ld;
    double *y = d.Y + row * ld;
    for (int j = lane; j < n; j += 64) bl[j] = br[j];
    wave_sync();
    const double sigma = sc->sigma;
    for (int i = lane; i < n; i += 64) {
        const double *ai = A + (size_t) i * ld;
        double dot = 0.;
        for (int l = 0; l < n; l++) dot += ai[l] * bl[l];
        y[i] = dot;
        const double mi = m[i];
        xm[i] = mi - sigma * dot;
        xp[i] = mi + sigma * dot;
    }
    wave_sync();
    if (d.X) {
        double *x0 = d.X + ((size_t) p * 2 * mu + r) * ld, *x1 = x0 + (size_t) mu * ld;
        for (int j = lane; j < n; j += 64) {
            x0[j] = xm[j];
            x1[j] = xp[j];
        }
    }
    if (c.obj < 0) return;      // a host objective evaluates X
    double f0 = eval_row_group<64>(c.obj, n, xm, d.aux, lane);
    double f1 = eval_row_group<64>(c.obj, n, xp, d.aux, lane);
    if (f0 != f0) f0 = HEES_INF;
    if (f1 != f1) f1 = HEES_INF;
    if (lane == 0) {
        d.f[(size_t) p * 2 * mu + r] = f0;
        d.f[(size_t) p * 2 * mu + mu + r] = f1;
    }
}

// The same on the fp64 matrix pipe: a workgroup per 16 rows, its wavefronts share the tiles of 16
// coordinates.  A tile of Y is 16 x 16 over K = n: the A operand is b[row][l], the B operand
// A[coordinate][l].  The candidates of the 16 rows wait in LDS (16 rows of m - sigma y, then 16 of
// m + sigma y); after the barrier a wavefront takes every fourth of them through the objective.
// grid (ceil(mu / 16), P), 256 threads, LDS 32 ld doubles
__global__ __launch_bounds__(256) void hees_points_mfma(HeesDev d, HeesConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const HeesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ar = lane & 15, ak = lane >> 4;
    const int n = c.n, ld = c.ld, mu = c.mu, r0 = blockIdx.x * 16;
    const size_t pb = (size_t) p * mu, pf = (size_t) p * 2 * mu;
    const double *A = d.A + (size_t) p * n * ld, *m = d.m + (size_t) p * ld;
    const double sigma = sc->sigma;
    const bool plive = r0 + ar < mu;
    const double *brow = d.b + (pb + min(r0 + ar, mu - 1)) * ld;
    for (int ct = wave; 16 * ct < n; ct += 4) {
        const int gi = ct * 16 + ar;
        const bool ilive = gi < n;
        const double *arow = A + (size_t) min(gi, n - 1) * ld;
        hees_d4 acc = { 0., 0., 0., 0. };
        for (int s = 0; 4 * s < n; s++) {
            const int l = 4 * s + ak;
            const double a = plive && l < n ? brow[l] : 0.;
            const double b = ilive && l < n ? arow[l] : 0.;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = ak + 4 * r;
            if (r0 + row < mu && ilive) {
                const double y = acc[r], mi = m[gi];
                d.Y[(pb + r0 + row) * ld + gi] = y;
                lds[(size_t) row * ld + gi] = mi - sigma * y;
                lds[(size_t) (16 + row) * ld + gi] = mi + sigma * y;
            }
        }
    }
    __syncthreads();
    for (int q = wave; q < 32; q += 4) {
        const int pt = r0 + (q & 15);
        if (pt >= mu) continue;
        const int idx = q < 16 ? pt : pt + mu;
        const double *x = lds + (size_t) q * ld;
        if (d.X) {
            double *xo = d.X + (pf + idx) * ld;
            for (int j = lane; j < n; j += 64) xo[j] = x[j];
        }
        if (c.obj < 0) continue;        // a host objective evaluates X
        double f = eval_row_group<64>(c.obj, n, x, d.aux, lane);
        if (f != f) f = HEES_INF;
        if (lane == 0) d.f[pf + idx] = f;
    }
}

// order[k] = the index of rank k among the 2 mu values, rank[i] = the rank of index i; ties to the
// lower index.  grid (ceil(2 mu / 32), P), 256 threads = 32 candidates x 8 slices
__global__ __launch_bounds__(256) void hees_rank(HeesDev d, HeesConst c)
{
    const int p = blockIdx.y;
    const HeesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    __shared__ __attribute__((aligned(16))) double tile[RANK_TILE];
    const int tid = threadIdx.x, cnt2 = 2 * c.mu;
    const int cand = blockIdx.x * 32 + (tid >> 3), slice = tid & 7;
    const size_t pf = (size_t) p * cnt2;
    const int cnt = rank_by_counting(d.f + pf, cnt2, cand, slice, tile);
    if (cand < cnt2 && slice == 0) {
        d.order[pf + cnt] = cand;
        d.rank[pf + cand] = cnt;
    }
}

// maximum over a workgroup of 256 threads through scratch[4], NaN never wins (std::max(a, b) keeps
// a unless a < b)
__device__ inline double hees_block_max(double v, double *scratch)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        v = v < ov ? ov : v;
    }
    __syncthreads();
    if ((tid & 63) == 0) scratch[tid >> 6] = v;
    __syncthreads();
    double s = scratch[0];
#pragma unroll
    for (int w = 1; w < 4; w++) s = s < scratch[w] ? scratch[w] : s;
    return s;
}

// The scalars of the covariance update (:262-292: h, max h, the trust region, q; the coefficient
// (q_i - 1) / (|z_i|^2 B) of row i in hees_adapt, or the note that A stays as it is), the
// differences dw_i = w_rank(i + mu) - w_rank(i), then m += sigma Y^T dw (= sum w x of :327-331,
// because sum w = 1), dz = b^T dw (:345-353), p_s, g_s and sigma (:354-363).  One workgroup per
// population, a thread per coordinate.  grid (P), 256 threads
__global__ __launch_bounds__(256) void hees_update(HeesDev d, HeesConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    HeesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    __shared__ double scratch[4];
    const int tid = threadIdx.x, n = c.n, ld = c.ld, mu = c.mu;
    const size_t pb = (size_t) p * mu, pf = (size_t) p * 2 * mu, pv = (size_t) p * ld;
    const double fm = sc->fm, sigma = sc->sigma, gs0 = sc->gs;
    double mx = -HEES_INF;
    for (int i = tid; i < mu; i += 256) {
        const double nz = d.norms[pb + i];
        const double h = (d.f[pf + i + mu] + d.f[pf + i] - 2. * fm) / (nz * nz);
        d.hess[pb + i] = h;
        mx = mx < h ? h : mx;
        d.dw[pb + i] = d.w[d.rank[pf + i + mu]] - d.w[d.rank[pf + i]];
    }
    const double maxh = hees_block_max(mx, scratch);
    const bool skip = maxh <= 0.;
    if (!skip) {
        const double ctrust = maxh / c.kappa;
        double part = 0.;
        for (int i = tid; i < mu; i += 256) {
            double h = d.hess[pb + i];
            h = h < ctrust ? ctrust : h;
            d.hess[pb + i] = h;
            const double lq = log(h);
            d.q[pb + i] = lq;
            part += lq / mu;
        }
        const double meanq = block_sum<4>(part, scratch);
        for (int i = tid; i < mu; i += 256) {
            const double nz = d.norms[pb + i];
            const double qq = exp((d.q[pb + i] - meanq) * (-c.etaA * 0.5));
            d.q[pb + i] = qq;
            d.coef[pb + i] = (qq - 1.) / (nz * nz * c.B);
        }
    }
    __syncthreads();    // dw (and the scalars above) are this workgroup's own writes
    double pss = 0.;
    for (int j = tid; j < n; j += 256) {
        double am = 0., dz = 0.;
        for (int i = 0; i < mu; i++) {
            const double w = d.dw[pb + i];
            am += d.Y[(pb + i) * ld + j] * w;
            dz += d.b[(pb + i) * ld + j] * w;
        }
        const double mj = d.m[pv + j];
        d.mprev[pv + j] = mj;
        d.m[pv + j] = mj + sigma * am;
        const double psj = (1. - c.cs) * d.ps[pv + j] + c.csc * dz;
        d.ps[pv + j] = psj;
        pss += psj * psj;
    }
    pss = block_sum<4>(pss, scratch);
    if (tid != 0) return;
    const double gs = ((1. - c.cs) * (1. - c.cs)) * gs0 + c.cs * (2. - c.cs);
    const double s = sqrt(pss) / c.chi - sqrt(gs);
    const double e = c.cs / c.ds * s;
    sc->gs = gs;
    sc->sigma_prev = sigma;
    sc->sigma = sigma * exp(e < 1. ? e : 1.);       // std::min(1., e)
    sc->maxh = maxh;
    sc->skip = skip ? 1 : 0;
}

// A += Y^T diag(coef) b, a 16 x 16 tile of A per workgroup, the rows i < mu staged through LDS
// sixteen at a time; left out when max h <= 0 (:271-273).  grid (ceil(n / 16), ceil(n / 16), P),
// 256 threads
__global__ __launch_bounds__(256) void hees_adapt(HeesDev d, HeesConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.z;
    const HeesScal *sc = d.scal + p;
    if (pop_frozen(c, sc) || sc->skip) return;
    __shared__ double sy[16][17], sb[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, n = c.n, ld = c.ld, mu = c.mu;
    const int r = blockIdx.y * 16 + ty, col = blockIdx.x * 16 + tx;
    const size_t pb = (size_t) p * mu;
    double acc = 0.;
    for (int i0 = 0; i0 < mu; i0 += 16) {
        const int i = i0 + ty, ry = blockIdx.y * 16 + tx;
        const bool live = i < mu;
        __syncthreads();
        sy[ty][tx] = live && ry < n ? d.coef[pb + i] * d.Y[(pb + i) * ld + ry] : 0.;
        sb[ty][tx] = live && col < n ? d.b[(pb + i) * ld + col] : 0.;
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 16; t++) acc += sy[t][ty] * sb[t][tx];
    }
    if (r < n && col < n) {
        double *a = d.A + ((size_t) p * n + r) * ld + col;
        *a = *a + acc;
    }
}

// The same on the fp64 matrix pipe: a 16 x 16 tile of A per workgroup over K = mu, the A operand
// coef_i Y[i][row], the B operand b[i][column]; the four wavefronts take every fourth step of four
// rows i and their partial tiles are added in a fixed order.
// grid (ceil(n / 16), ceil(n / 16), P), 256 threads
__global__ __launch_bounds__(256) void hees_adapt_mfma(HeesDev d, HeesConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.z;
    const HeesScal *sc = d.scal + p;
    if (pop_frozen(c, sc) || sc->skip) return;
    __shared__ double part[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ar = lane & 15, ak = lane >> 4;
    const int n = c.n, ld = c.ld, mu = c.mu;
    const int gi = blockIdx.y * 16 + ar, gj = blockIdx.x * 16 + ar;
    const size_t pb = (size_t) p * mu;
    hees_d4 acc = { 0., 0., 0., 0. };
    for (int s = wave; 4 * s < mu; s += 4) {
        const int i = 4 * s + ak;
        const bool live = i < mu;
        const size_t row = (pb + min(i, mu - 1)) * ld;
        const double a = live && gi < n ? d.coef[pb + i] * d.Y[row + gi] : 0.;
        const double b = live && gj < n ? d.b[row + gj] : 0.;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) part[wave][r * 64 + lane] = acc[r];
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int q = r * 64 + lane;
        const double v = ((part[0][q] + part[1][q]) + part[2][q]) + part[3][q];
        const int i = blockIdx.y * 16 + ak + 4 * r, j = blockIdx.x * 16 + ar;
        if (i < n && j < n) {
            double *a = d.A + ((size_t) p * n + i) * ld + j;
            *a = *a + v;
        }
    }
}

// f(m) (:332-333; a host objective has left it in fmh), the incumbent, which follows the means
// alone (:336-339), it++, fev += 2 mu + 1, converged() (:366-382: the spread of the 2 mu values as
// a two-pass sum) and the stop flag.  init_only: the state after init()
// (:62-66), where the 2 mu values are still zeros.  grid (P), 256 threads
__global__ __launch_bounds__(256) void hees_finish(HeesDev d, HeesConst c, int init_only)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    HeesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    __shared__ double sm[HEES_MAX_N];
    __shared__ double scratch[4];
    const int tid = threadIdx.x, lane = tid & 63, n = c.n, cnt2 = 2 * c.mu;
    const size_t pf = (size_t) p * cnt2, pv = (size_t) p * c.ld;
    const double fbest0 = sc->fbest;
    for (int j = tid; j < n; j += 256) sm[j] = d.m[pv + j];
    __syncthreads();
    double fm;
    if (c.obj >= 0) {
        fm = eval_row_group<64>(c.obj, n, sm, d.aux, lane);     // (every wavefront: the same bits)
        if (fm != fm) fm = HEES_INF;
    } else {
        fm = d.fmh[p];
    }
    double s = 0.;
    for (int i = tid; i < cnt2; i += 256) s += d.f[pf + i];
    const double mean = block_sum<4>(s, scratch) / cnt2;
    double m2 = 0.;
    for (int i = tid; i < cnt2; i += 256) {
        const double dd = d.f[pf + i] - mean;
        m2 += dd * dd;
    }
    m2 = block_sum<4>(m2, scratch);
    const bool take = init_only || fm < fbest0;
    if (take)
        for (int j = tid; j < n; j += 256) d.xbest[pv + j] = sm[j];
    if (tid != 0) return;
    sc->fm = fm;
    if (take) sc->fbest = fm;
    sc->m2 = m2;
    const int conv = m2 <= cnt2 * c.tol * c.tol ? 1 : 0;
    sc->conv = conv;
    if (init_only) return;
    sc->it++;
    sc->gen++;
    sc->fev += cnt2 + 1;
    // optimize(), :143-149: converged() ends the loop, else its head looks at the budget
    if (conv) sc->stop = 1;
    else if (sc->fev >= c.mfev) sc->stop = 2;
}

} // namespace bbo
