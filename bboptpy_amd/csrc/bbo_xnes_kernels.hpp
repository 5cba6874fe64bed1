// bbo_xnes_kernels.hpp -- one xNES generation as gfx950 kernels (grid.y or .x = population).
//
//   kernel            reference lines (xnes.cpp)                                work per population
//   xnes_draw         :113-116 the normals of the np rows                        np n / 4 Philox calls
//                     (xnes_settle: the draws the fast test left open;
//                     xnes_take: the same rows from an injected table)
//   xnes_points       :117-123 Y = Z B^T, x = mu + sigma y, the objective        2 np n^2 flops
//                     (xnes_points_mfma from n = 16 on: B streams in once)
//   xnes_rank         :128 (rank by counting; ties to the lower index)           np^2 compares
//   xnes_step         :131-171 mu, G_sigma, sigma, the stop test; the operator   low-rank np^2 n + O(np^3),
//                     of the update of B (bbo_xnes.hpp)                          dense np n^2 + O(n^3), n <= 31
//   xnes_adapt_lr     :174-190 B <- e^{-c G_sigma} (B + Y^T Q), Q = H Z          2 np n^2 flops
//   xnes_adapt_dense  the same as B <- B E                                       2 n^3 flops, n <= 31
#pragma once

#include "bbo_xnes.hpp"
#include "bbo_objectives.hpp"
#include "bbo_rng.hpp"
#include "bbo_wave.hpp"

namespace bbo {

#define XNES_INF (__builtin_huge_val())

// v_mfma_f64_16x16x4_f64, operands as in bbo_hees_kernels.hpp: A[row = lane & 15][k = lane >> 4],
// B[k = lane >> 4][col = lane & 15], C/D four doubles per lane, col = lane & 15, row = (lane >> 4) + 4 reg
typedef double xnes_d4 __attribute__((ext_vector_type(4)));

// The rows of Z: a wavefront per row, lane q takes the Philox call (row, q, generation, population)
// -- four ziggurat normals, columns 4 q .. 4 q + 3.  Two kernels for the reason hees_draw gives: the
// first forms the fast-path candidate of every word and leaves a NaN where the fast test did not
// settle the draw, the second finds those and takes the slow path with the seed read per lane.
// grid (ceil(np / 4), P), 256 threads, both
__global__ __launch_bounds__(256) void xnes_draw(XnesDev d, XnesConst c)
{
    const int p = blockIdx.y;
    const XnesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave, n = c.n;
    if (r >= c.np) return;
    double *z = d.Z + ((size_t) p * c.np + r) * c.ld;
    const uint32_t gen = (uint32_t) sc->gen, sw = stream_word(STREAM_XNES_NORMAL, (uint32_t) p);
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

__global__ __launch_bounds__(256) void xnes_settle(XnesDev d, XnesConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const XnesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave, n = c.n;
    if (r >= c.np) return;
    double *z = d.Z + ((size_t) p * c.np + r) * c.ld;
    const uint32_t gen = (uint32_t) sc->gen, sw = stream_word(STREAM_XNES_NORMAL, (uint32_t) p);
    const uint64_t seed = d.lane_seed[lane];
    for (int j = lane; j < n; j += 64) {
        if (z[j] == z[j]) continue;
        const uint32_t q = (uint32_t) j >> 2, slot = (uint32_t) j & 3u;
        const u32x4 w4 = philox4x32_10(seed, (uint32_t) r, q, gen, sw);
        const uint32_t lo = (slot & 1u) ? w4.y : w4.x, hi = (slot & 1u) ? w4.w : w4.z;
        const uint32_t w = (slot & 2u) ? hi : lo;
        [[clang::always_inline]] z[j] = zig_slow(seed, (uint32_t) r, q, slot, gen, sw, w & 1023u, (w >> 10) | 1u,
                (w >> 10) & 1u, zig_global_wk(), zig_global_f());
    }
}

// The same rows from the caller's table.  grid (ceil(np / 4), P), 256 threads
__global__ __launch_bounds__(256) void xnes_take(XnesDev d, XnesConst c)
{
    const int p = blockIdx.y;
    const XnesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave;
    if (r >= c.np) return;
    const size_t row = ((size_t) p * c.np + r) * c.ld;
    for (int j = lane; j < c.n; j += 64) d.Z[row + j] = d.zin[row + j];
}

// B = I, order = rank = identity (the buffers arrive zeroed).  grid (P), 256 threads
__global__ __launch_bounds__(256) void xnes_eye(XnesDev d, XnesConst c)
{
    const int p = blockIdx.x;
    double *B = d.B + (size_t) p * c.n * c.ld;
    for (int i = threadIdx.x; i < c.n; i += 256) B[(size_t) i * c.ld + i] = 1.;
    if ((int) threadIdx.x < c.np) {
        d.order[(size_t) p * c.np + threadIdx.x] = threadIdx.x;
        d.rank[(size_t) p * c.np + threadIdx.x] = threadIdx.x;
    }
}

// Y = Z B^T and the candidates below one tile of coordinates: a wavefront per row r.  The row z_r
// waits in LDS, lane i forms y_i = B_i . z_r in the reference's order (:119-121), x = mu + sigma y
// goes to LDS, to X, and through the objective.  grid (ceil(np / 4), P), 256 threads, LDS 8 ld doubles
__global__ __launch_bounds__(256) void xnes_points(XnesDev d, XnesConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const XnesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave, n = c.n, ld = c.ld;
    if (r >= c.np) return;
    const size_t row = ((size_t) p * c.np + r) * ld;
    double *zl = lds + (size_t) wave * 2 * ld, *xl = zl + ld;
    const double *B = d.B + (size_t) p * n * ld, *mu = d.mu + (size_t) p * ld;
    for (int j = lane; j < n; j += 64) zl[j] = d.Z[row + j];
    wave_sync();
    const double sigma = sc->sigma;
    for (int i = lane; i < n; i += 64) {
        const double *bi = B + (size_t) i * ld;
        double dot = 0.;
        for (int l = 0; l < n; l++) dot += bi[l] * zl[l];
        d.Y[row + i] = dot;
        const double x = mu[i] + sigma * dot;
        xl[i] = x;
        d.X[row + i] = x;
    }
    wave_sync();
    if (c.obj < 0) return;      // a host objective evaluates X
    double f = eval_row_group<64>(c.obj, n, xl, d.aux, lane);
    if (f != f) f = XNES_INF;
    if (lane == 0) d.f[(size_t) p * c.np + r] = f;
}

// The same on the fp64 matrix pipe: a workgroup per population, its wavefronts share the tiles of 16
// coordinates.  A tile of Y is 16 x 16 over K = n: the A operand is Z[row][l], the B operand
// B[coordinate][l]; np <= 22 rows are one or two row tiles, and both take the same B fragment, so B
// streams in once.  The candidates wait in LDS; after the barrier a wavefront takes every fourth of
// them through the objective.  grid (P), 256 threads, LDS np ld doubles
__global__ __launch_bounds__(256) void xnes_points_mfma(XnesDev d, XnesConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    const XnesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ar = lane & 15, ak = lane >> 4;
    const int n = c.n, ld = c.ld, np = c.np;
    const size_t pb = (size_t) p * np;
    const double *B = d.B + (size_t) p * n * ld, *mu = d.mu + (size_t) p * ld;
    const double sigma = sc->sigma;
    const bool two = np > 16, live0 = ar < np, live1 = 16 + ar < np;
    const double *zrow0 = d.Z + (pb + min(ar, np - 1)) * ld, *zrow1 = d.Z + (pb + min(16 + ar, np - 1)) * ld;
    for (int ct = wave; 16 * ct < n; ct += 4) {
        const int gi = ct * 16 + ar;
        const bool ilive = gi < n;
        const double *brow = B + (size_t) min(gi, n - 1) * ld;
        xnes_d4 acc0 = { 0., 0., 0., 0. }, acc1 = { 0., 0., 0., 0. };
        for (int s = 0; 4 * s < n; s++) {
            const int l = 4 * s + ak;
            const double b = ilive && l < n ? brow[l] : 0.;
            const double a0 = live0 && l < n ? zrow0[l] : 0.;
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc0, 0, 0, 0);
            if (two) {
                const double a1 = live1 && l < n ? zrow1[l] : 0.;
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < 2; t++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = 16 * t + ak + 4 * r;
                if (row < np && ilive) {
                    const double y = t ? acc1[r] : acc0[r], x = mu[gi] + sigma * y;
                    d.Y[(pb + row) * ld + gi] = y;
                    d.X[(pb + row) * ld + gi] = x;
                    lds[(size_t) row * ld + gi] = x;
                }
            }
        }
    }
    __syncthreads();
    if (c.obj < 0) return;          // a host objective evaluates X
    for (int q = wave; q < np; q += 4) {
        double f = eval_row_group<64>(c.obj, n, lds + (size_t) q * ld, d.aux, lane);
        if (f != f) f = XNES_INF;
        if (lane == 0) d.f[pb + q] = f;
    }
}

// order[k] = the index of rank k among the np values, rank[i] = the rank of index i; ties to the
// lower index.  One wavefront, a lane per candidate.  grid (P), 64 threads
__global__ __launch_bounds__(64) void xnes_rank(XnesDev d, XnesConst c)
{
    const int p = blockIdx.x;
    const XnesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int i = threadIdx.x, np = c.np;
    if (i >= np) return;
    const double *f = d.f + (size_t) p * np;
    const double fi = f[i];
    int cnt = 0;
    for (int j = 0; j < np; j++) {
        const double fj = f[j];
        cnt += (fj < fi || (fj == fi && j < i)) ? 1 : 0;
    }
    d.order[(size_t) p * np + cnt] = i;
    d.rank[(size_t) p * np + i] = cnt;
}

// Cyclic Jacobi for a symmetric m x m matrix in LDS (m <= 32, leading dimension 33), one workgroup of
// 256 threads.  A sweep is the round-robin schedule of m - 1 rounds (m rounded up to even; the
// pairs of the padding index rest), each round rotates its m / 2 disjoint pairs together: the
// angles from the matrix as it stands, then A <- A J (columns), A <- J^T A (rows) and V <- V J, a
// barrier between.  A pair is rotated while |a_pq| > 2^-52 |A|_F (the norm before the first sweep);
// the sweeps end with the first that rotates nothing, 30 at the most.  The order is fixed, so the
// result is the same bits on every run.  On return diag(a) holds the eigenvalues (unsorted), the
// columns of v the eigenvectors.
__device__ inline void xnes_jacobi(double *a, double *v, int m, double *scratch)
{
#pragma clang fp contract(off)
    __shared__ double cs[16], sn[16];
    __shared__ int pp[16], qq[16], rot;
    const int tid = threadIdx.x;
    double s = 0.;
    for (int idx = tid; idx < m * m; idx += 256) {
        const int i = idx / m, j = idx % m;
        v[i * XNES_EIG_LD + j] = i == j ? 1. : 0.;
        s += a[i * XNES_EIG_LD + j] * a[i * XNES_EIG_LD + j];
    }
    const double thr = sqrt(block_sum<4>(s, scratch)) * 0x1p-52;
    __syncthreads();
    if (m < 2) return;
    const int me = (m + 1) & ~1, half = me / 2, rounds = me - 1;
    for (int sweep = 0; sweep < 30; sweep++) {
        if (tid == 0) rot = 0;
        __syncthreads();
        for (int r = 0; r < rounds; r++) {
            if (tid < half) {
                int p = tid == 0 ? me - 1 : (r + tid) % rounds;
                int q = tid == 0 ? r : (r + rounds - tid) % rounds;
                if (p > q) {
                    const int t = p;
                    p = q;
                    q = t;
                }
                double co = 1., si = 0.;
                if (q < m) {
                    const double apq = a[p * XNES_EIG_LD + q];
                    if (fabs(apq) > thr) {
                        const double app = a[p * XNES_EIG_LD + p], aqq = a[q * XNES_EIG_LD + q];
                        const double theta = (aqq - app) / (2. * apq);
                        const double t = copysign(1., theta) / (fabs(theta) + sqrt(theta * theta + 1.));
                        co = 1. / sqrt(t * t + 1.);
                        si = t * co;
                        rot = 1;
                    }
                }
                cs[tid] = co;
                sn[tid] = si;
                pp[tid] = p;
                qq[tid] = q;
            }
            __syncthreads();
            for (int idx = tid; idx < half * m; idx += 256) {
                const int t = idx / m, k = idx % m, p = pp[t], q = qq[t];
                const double co = cs[t], si = sn[t];
                if (si == 0.) continue;
                const double akp = a[k * XNES_EIG_LD + p], akq = a[k * XNES_EIG_LD + q];
                a[k * XNES_EIG_LD + p] = co * akp - si * akq;
                a[k * XNES_EIG_LD + q] = si * akp + co * akq;
                const double vkp = v[k * XNES_EIG_LD + p], vkq = v[k * XNES_EIG_LD + q];
                v[k * XNES_EIG_LD + p] = co * vkp - si * vkq;
                v[k * XNES_EIG_LD + q] = si * vkp + co * vkq;
            }
            __syncthreads();
            for (int idx = tid; idx < half * m; idx += 256) {
                const int t = idx / m, k = idx % m, p = pp[t], q = qq[t];
                const double co = cs[t], si = sn[t];
                if (si == 0.) continue;
                const double apk = a[p * XNES_EIG_LD + k], aqk = a[q * XNES_EIG_LD + k];
                a[p * XNES_EIG_LD + k] = k == q ? 0. : co * apk - si * aqk;
                a[q * XNES_EIG_LD + k] = k == p ? 0. : si * apk + co * aqk;
            }
            __syncthreads();
        }
        const bool done = rot == 0;
        __syncthreads();
        if (done) break;
    }
}

// The small step: one workgroup per population, everything in ranked order through order[].
//   mu += eta_mu sigma Y^T u                       (:131-136, :164-168: B G_delta = sum u_i y_i)
//   G_sigma = sum_k u_k |z_k|^2 / n                (:138-154; sum u = 0 drops the -1)
//   sigma *= exp(eta_sigma G_sigma / 2), the best ever seen, it, fev, the stop test (:171, :211-219)
// then the operator of the update of B, c = eta_B / 2:
//   low-rank  K = Zs Zs^T (a wavefront per pair of rows, lanes over the coordinates, one butterfly),
//             K = L L^T by one wavefront (a lane per row), S = L^T U L, S = W Lambda W^T (xnes_jacobi),
//             T = L^-T W, H = T (e^{c Lambda} - 1) T^T, and Q = Hs Z with Hs = H taken back to the
//             sampling order.  A pivot that is not finite or not above 2^-40 K_jj (two equal or
//             dependent rows) leaves B alone for this generation: skip = 1, fact_fail++.
//   dense     G_B = Zs^T U Zs - G_sigma I, G_B = V Lambda V^T (xnes_jacobi), E = V e^{c Lambda} V^T.
// grid (P), 256 threads
__global__ __launch_bounds__(256) void xnes_step(XnesDev d, XnesConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    XnesScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    constexpr int LD = XNES_EIG_LD;
    __shared__ double sa[XNES_EIG_MAX * LD], sv[XNES_EIG_MAX * LD], sl[XNES_EIG_MAX * LD], st[XNES_EIG_MAX * LD];
    __shared__ double su[XNES_NPP], snz[XNES_NPP], sev[XNES_EIG_MAX], scratch[4];
    __shared__ int sord[XNES_NPP], sfail;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = c.n, ld = c.ld, np = c.np;
    const size_t pb = (size_t) p * np, pv = (size_t) p * ld;
    const double sigma = sc->sigma, fbest0 = sc->fbest;
    if (tid < XNES_NPP) {
        sord[tid] = tid < np ? d.order[pb + tid] : 0;
        su[tid] = tid < np ? d.u[tid] : 0.;
    }
    __syncthreads();
    const double step = c.etamu * sigma;
    for (int j = tid; j < n; j += 256) {
        double gd = 0.;
        for (int k = 0; k < np; k++) gd += su[k] * d.Y[(pb + sord[k]) * ld + j];
        d.mu[pv + j] = d.mu[pv + j] + step * gd;
    }
    for (int k = wave; k < np; k += 4) {
        const double *z = d.Z + (pb + sord[k]) * ld;
        double s = 0.;
        for (int j = lane; j < n; j += 64) s += z[j] * z[j];
        s = group_sum<64>(s);
        if (lane == 0) snz[k] = s;
    }
    __syncthreads();
    const double fb = d.f[pb + sord[0]], fw = d.f[pb + sord[np - 1]];
    const bool take = fb < fbest0;
    if (take)
        for (int j = tid; j < n; j += 256) d.xbest[pv + j] = d.X[(pb + sord[0]) * ld + j];
    double gs = 0.;
    for (int k = 0; k < np; k++) gs += su[k] * snz[k];
    gs = gs / n;
    const double c2 = 0.5 * c.etab;
    if (tid == 0) {
        sc->gsigma = gs;
        sc->sigma = sigma * exp(0.5 * c.etasigma * gs);
        sc->escale = exp(-c2 * gs);
        if (take) sc->fbest = fb;
        const int conv = fabs(fb - fw) < c.tol ? 1 : 0;
        sc->conv = conv;
        sc->it++;
        sc->gen++;
        sc->fev += np;
        // optimize(), :201-207: converged() ends the loop, else its head looks at the budget
        if (conv) sc->stop = 1;
        else if (sc->fev >= c.mfev) sc->stop = 2;
        sfail = 0;
    }

    if (!c.lowrank) {
        // (n <= 31 here, np <= 14)
        for (int idx = tid; idx < np * n; idx += 256) {
            const int k = idx / n, j = idx % n;
            st[k * LD + j] = d.Z[(pb + sord[k]) * ld + j];
        }
        __syncthreads();
        for (int idx = tid; idx < n * n; idx += 256) {
            const int i = idx / n, j = idx % n;
            if (i > j) continue;
            double s = 0.;
            for (int k = 0; k < np; k++) s += su[k] * (st[k * LD + i] * st[k * LD + j]);
            if (i == j) s = s - gs;
            sa[i * LD + j] = s;
            sa[j * LD + i] = s;
        }
        __syncthreads();
        xnes_jacobi(sa, sv, n, scratch);
        if (tid < n) sev[tid] = exp(c2 * sa[tid * LD + tid]);
        __syncthreads();
        double *E = d.E + (size_t) p * XNES_EIG_MAX * XNES_EIG_MAX;
        for (int idx = tid; idx < n * n; idx += 256) {
            const int i = idx / n, j = idx % n;
            if (i > j) continue;
            double s = 0.;
            for (int k = 0; k < n; k++) s += (sv[i * LD + k] * sev[k]) * sv[j * LD + k];
            E[i * XNES_EIG_MAX + j] = s;
            E[j * XNES_EIG_MAX + i] = s;
        }
        if (tid == 0) sc->skip = 0;
        return;
    }

    for (int q = wave; q < np * np; q += 4) {
        const int a = q / np, b = q % np;
        if (a > b) continue;
        const double *za = d.Z + (pb + sord[a]) * ld, *zb = d.Z + (pb + sord[b]) * ld;
        double s = 0.;
        for (int j = lane; j < n; j += 64) s += za[j] * zb[j];
        s = group_sum<64>(s);
        if (lane == 0) {
            sl[a * LD + b] = s;
            sl[b * LD + a] = s;
        }
    }
    __syncthreads();
    if (wave == 0) {
        bool ok = true;
        for (int j = 0; j < np; j++) {
            const double kjj = sl[j * LD + j];
            double piv = kjj;
            for (int k = 0; k < j; k++) piv -= sl[j * LD + k] * sl[j * LD + k];
            if (!(piv > kjj * 0x1p-40) || !(piv < XNES_INF)) {
                ok = false;
                break;
            }
            const double ljj = sqrt(piv);
            if (lane > j && lane < np) {
                double s = sl[lane * LD + j];
                for (int k = 0; k < j; k++) s -= sl[lane * LD + k] * sl[j * LD + k];
                sl[lane * LD + j] = s / ljj;
            }
            wave_sync();
            if (lane == 0) sl[j * LD + j] = ljj;
            wave_sync();
        }
        if (lane == 0 && !ok) sfail = 1;
    }
    __syncthreads();
    if (sfail) {
        if (tid == 0) {
            sc->skip = 1;
            sc->fact_fail++;
        }
        return;
    }
    for (int idx = tid; idx < np * np; idx += 256) {
        const int a = idx / np, b = idx % np;
        if (a > b) continue;
        double s = 0.;
        for (int k = b; k < np; k++) s += (sl[k * LD + a] * su[k]) * sl[k * LD + b];
        sa[a * LD + b] = s;
        sa[b * LD + a] = s;
    }
    __syncthreads();
    xnes_jacobi(sa, sv, np, scratch);
    if (tid < np) sev[tid] = expm1(c2 * sa[tid * LD + tid]);
    __syncthreads();
    if (tid < np) {
        // L^T T = W, column tid by back substitution
        for (int i = np - 1; i >= 0; i--) {
            double s = sv[i * LD + tid];
            for (int k = i + 1; k < np; k++) s -= sl[k * LD + i] * st[k * LD + tid];
            st[i * LD + tid] = s / sl[i * LD + i];
        }
    }
    for (int idx = tid; idx < XNES_NPP * LD; idx += 256) sa[idx] = 0.;
    __syncthreads();
    for (int idx = tid; idx < np * np; idx += 256) {
        const int a = idx / np, b = idx % np;
        if (a > b) continue;
        double s = 0.;
        for (int k = 0; k < np; k++) s += (st[a * LD + k] * sev[k]) * st[b * LD + k];
        sa[sord[a] * LD + sord[b]] = s;
        sa[sord[b] * LD + sord[a]] = s;
    }
    __syncthreads();
    for (int j = tid; j < n; j += 256) {
        double zc[XNES_NPP];
#pragma unroll
        for (int t = 0; t < XNES_NPP; t++) zc[t] = t < np ? d.Z[(pb + t) * ld + j] : 0.;
        for (int i = 0; i < np; i++) {
            double s = 0.;
#pragma unroll
            for (int t = 0; t < XNES_NPP; t++) s += sa[i * LD + t] * zc[t];
            d.Q[(pb + i) * ld + j] = s;
        }
    }
    if (tid == 0) sc->skip = 0;
}

// B <- e^{-c G_sigma} (B + Y^T Q) on the fp64 matrix pipe, one pass over B: a workgroup per 16 rows of
// B, its wavefronts take every fourth tile of 16 columns; a tile is 16 x 16 over K = np (six steps of
// four at the most, the rows above np are zeros): the A operand Y[k][row] is read once per
// wavefront, the B operand Q[k][column] per tile.  grid (ceil(n / 16), P), 256 threads
__global__ __launch_bounds__(256) void xnes_adapt_lr(XnesDev d, XnesConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const XnesScal *sc = d.scal + p;
    if (pop_frozen(c, sc) || sc->skip) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ar = lane & 15, ak = lane >> 4;
    const int n = c.n, ld = c.ld, np = c.np;
    const size_t pb = (size_t) p * np;
    const double esc = sc->escale;
    const int gi = blockIdx.x * 16 + ar;
    double a[XNES_NPP / 4];
#pragma unroll
    for (int s = 0; s < XNES_NPP / 4; s++) {
        const int k = 4 * s + ak;
        a[s] = k < np && gi < n ? d.Y[(pb + min(k, np - 1)) * ld + min(gi, n - 1)] : 0.;
    }
    double *B = d.B + (size_t) p * n * ld;
    for (int ct = wave; 16 * ct < n; ct += 4) {
        const int gj = ct * 16 + ar;
        xnes_d4 acc = { 0., 0., 0., 0. };
#pragma unroll
        for (int s = 0; s < XNES_NPP / 4; s++) {
            const int k = 4 * s + ak;
            const double b = k < np && gj < n ? d.Q[(pb + min(k, np - 1)) * ld + min(gj, n - 1)] : 0.;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int i = blockIdx.x * 16 + ak + 4 * r;
            if (i < n && gj < n) {
                double *e = B + (size_t) i * ld + gj;
                *e = esc * (*e + acc[r]);
            }
        }
    }
}

// B <- B E below the low-rank route (n <= 31): B and E wait in LDS, a thread per entry, the sum in
// the reference's order (:180-187).  grid (P), 256 threads
__global__ __launch_bounds__(256) void xnes_adapt_dense(XnesDev d, XnesConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    const XnesScal *sc = d.scal + p;
    if (pop_frozen(c, sc) || sc->skip) return;
    __shared__ double sb[XNES_EIG_MAX * XNES_EIG_LD], se[XNES_EIG_MAX * XNES_EIG_LD];
    const int tid = threadIdx.x, n = c.n, ld = c.ld;
    double *B = d.B + (size_t) p * n * ld;
    const double *E = d.E + (size_t) p * XNES_EIG_MAX * XNES_EIG_MAX;
    for (int idx = tid; idx < n * n; idx += 256) {
        const int i = idx / n, j = idx % n;
        sb[i * XNES_EIG_LD + j] = B[(size_t) i * ld + j];
        se[i * XNES_EIG_LD + j] = E[i * XNES_EIG_MAX + j];
    }
    __syncthreads();
    for (int idx = tid; idx < n * n; idx += 256) {
        const int i = idx / n, j = idx % n;
        double s = 0.;
        for (int k = 0; k < n; k++) s += sb[i * XNES_EIG_LD + k] * se[k * XNES_EIG_LD + j];
        B[(size_t) i * ld + j] = s;
    }
}

} // namespace bbo
