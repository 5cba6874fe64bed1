// bbo_amalgam_kernels.hpp -- one (i)AMaLGaM generation as gfx950 kernels (grid.y or .z = population).
//
//   kernel            reference lines (amalgam.cpp)                             work per population
//   amalgam_init      :137-146 the uniform population in the box, its values    np n / 2 Philox calls
//   amalgam_init_mom  :161-174 mu and the diagonal of cov (the loop as written)  2 ss n
//   amalgam_mean      :364-370, :384-399 mu, mushift, the elite                  ss n
//   amalgam_gram      :373-382 centred Gram of the ranked rows, lower tiles      ss n^2 flops (fp64 MFMA)
//   amalgam_cov       the slabs in order, the blend with the old cov, mirrored   slabs n^2 / 2
//   amalgam_factor    :401-415, :455-528 dchdc, no pivoting, panels of 16        n^3 / 3 flops
//   amalgam_draw      :421-424 (amalgam_settle, amalgam_take)                    np n / 4 Philox calls
//   amalgam_points    :425-429 X = mu + Z chol^T, lower tiles of chol only       np n^2 flops (fp64 MFMA)
//   amalgam_eval      :434-451 the shifted rows, the objective of rows 1..       np - 1 evaluations
//   amalgam_adapt     :213-233, :290-356 SDR, multiplier, counters, stop tests   np n + n^2 / 2
//   amalgam_rank      :361 by counting, ties to the lower index                  np^2 compares
#pragma once

#include "bbo_amalgam.hpp"
#include "bbo_objectives.hpp"
#include "bbo_rank.hpp"
#include "bbo_rng.hpp"
#include "bbo_wave.hpp"

namespace bbo {

#define AMALGAM_INF (__builtin_huge_val())

// v_mfma_f64_16x16x4_f64: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15], C/D four
// doubles per lane, col = lane & 15, row = (lane >> 4) + 4 reg
typedef double amalgam_d4 __attribute__((ext_vector_type(4)));

__device__ inline uint32_t amalgam_sub(const AmalgamConst &c, int p)
{
    return (uint32_t) (c.sub0 + p);
}

// One wavefront evaluates the row it has just written (x in LDS).  A NaN ranks last.
__device__ inline double amalgam_objective(const AmalgamConst &c, const AmalgamDev &d, const double *xl, int lane)
{
    double f = eval_row_group<64>(c.obj, c.n, xl, d.aux, lane);
    if (f != f) f = AMALGAM_INF;
    return f;
}

// The initial population: a wavefront per row, lane q takes the Philox call (row, q, 0, population)
// -- two uniforms, columns 2 q and 2 q + 1 -- or the row of the injected table; then the objective.
// grid (ceil(np / 4), P), 256 threads, LDS 4 ld doubles
__global__ __launch_bounds__(256) void amalgam_init(AmalgamDev d, AmalgamConst c, const double *xin)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int p = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave, n = c.n, ld = c.ld;
    if (r >= c.np) return;
    const size_t row = ((size_t) p * c.np + r) * ld;
    double *xl = lds + (size_t) wave * ld;
    if (xin) {
        for (int j = lane; j < n; j += 64) xl[j] = xin[row + j];
    } else {
        const uint32_t sw = stream_word(STREAM_AMALGAM_INIT, amalgam_sub(c, p));
        for (int q = lane; 2 * q < n; q += 64) {
            const u32x4 w = philox4x32_10(c.seed, (uint32_t) r, (uint32_t) q, 0u, sw);
            const double u[2] = { u01(w.x, w.y), u01(w.z, w.w) };
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int j = 2 * q + t;
                if (j < n) xl[j] = d.lower[j] + u[t] * (d.upper[j] - d.lower[j]);
            }
        }
    }
    wave_sync();
    for (int j = lane; j < n; j += 64) d.X[row + j] = xl[j];
    if (c.obj < 0) return;      // a host objective evaluates X
    const double f = amalgam_objective(c, d, xl, lane);
    if (lane == 0) d.f[(size_t) p * c.np + r] = f;
}

// order[k] = the row of rank k, rank[i] = the rank of row i; ties to the lower index.
// grid (ceil(np / 32), P), 256 threads
__global__ __launch_bounds__(256) void amalgam_rank(AmalgamDev d, AmalgamConst c)
{
    const int p = blockIdx.y;
    if (pop_frozen(c, d.scal + p)) return;
    __shared__ double tile[RANK_TILE];
    const int cand = blockIdx.x * 32 + (threadIdx.x >> 3), slice = threadIdx.x & 7;
    const size_t pb = (size_t) p * c.np;
    const int r = rank_by_counting<8>(d.f + pb, c.np, cand, slice, tile);
    if (cand < c.np && slice == 0) {
        d.order[pb + r] = cand;
        d.rank[pb + cand] = r;
    }
}

// mu = (sum of the best ss rows) / ss and the diagonal of cov by the loop of :168-174, which divides
// by ss inside the sum; the counters of a fresh population.  grid (P), 256 threads
__global__ __launch_bounds__(256) void amalgam_init_mom(AmalgamDev d, AmalgamConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x, tid = threadIdx.x, n = c.n, ld = c.ld, ss = c.ss;
    const size_t pb = (size_t) p * c.np, pv = (size_t) p * ld;
    const int *ord = d.order + pb;
    double *cov = d.cov + (size_t) p * ld * ld;
    const double inv = 1. / ss;
    for (int j = tid; j < n; j += 256) {
        double m = 0.;
        for (int k = 0; k < ss; k++) m += d.X[(pb + ord[k]) * ld + j];
        m *= inv;
        d.mu[pv + j] = m;
        double v = 0.;
        for (int k = 0; k < ss; k++) {
            const double xm = d.X[(pb + ord[k]) * ld + j] - m;
            v += xm * xm;
            v /= ss;
        }
        cov[(size_t) j * ld + j] = v;
        d.xbest[pv + j] = d.X[(pb + ord[0]) * ld + j];
    }
    if (tid == 0) {
        AmalgamScal *sc = d.scal + p;
        sc->fbest = d.f[pb + ord[0]];
        sc->felite = sc->fbest;
        sc->fev = c.np;
    }
}

// The mean of the ranked rows in the reference's order of additions, the anticipated mean shift and
// the elite (the row of rank 0 and its value, which the sampler carries over).  grid (P), 256 threads
__global__ __launch_bounds__(256) void amalgam_mean(AmalgamDev d, AmalgamConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    AmalgamScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int tid = threadIdx.x, n = c.n, ld = c.ld, ss = c.ss, t = sc->t;
    const size_t pb = (size_t) p * c.np, pv = (size_t) p * ld;
    const int *ord = d.order + pb;
    const double w = 1. / ss;
    for (int j = tid; j < n; j += 256) {
        const double old = d.mu[pv + j];
        double m = 0.;
        for (int k = 0; k < ss; k++) m += w * d.X[(pb + ord[k]) * ld + j];
        d.muold[pv + j] = old;
        d.mu[pv + j] = m;
        double sh = 0.;
        if (t == 1) sh = m - old;
        else if (t > 1) {
            sh = d.mushift[pv + j] * (1. - c.etashift);
            sh += c.etashift * (m - old);
        }
        d.mushift[pv + j] = sh;
        d.xelite[pv + j] = d.X[(pb + ord[0]) * ld + j];
    }
    if (tid == 0) sc->felite = d.f[pb + ord[0]];
}

// The centred Gram of the ranked rows, G_ij = sum_m (x_mi - mu_i)(x_mj - mu_j), tiles on and below the
// diagonal: a wavefront per 16 x 16 tile and slab of AMALGAM_SLAB ranked rows, K in steps of 4, the
// rows gathered through order[].  No atomics: a slab writes its own image.
// grid (ceil(tiles / 4), slabs, P), 256 threads
__global__ __launch_bounds__(256) void amalgam_gram(AmalgamDev d, AmalgamConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.z, slab = blockIdx.y;
    if (pop_frozen(c, d.scal + p)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ar = lane & 15, ak = lane >> 4;
    const int n = c.n, ld = c.ld, T = (n + 15) / 16;
    const int tl = blockIdx.x * 4 + wave;
    if (tl >= T * (T + 1) / 2) return;
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= tl) ti++;
    const int tj = tl - ti * (ti + 1) / 2;
    const size_t pb = (size_t) p * c.np;
    const int *ord = d.order + pb;
    const double *mu = d.mu + (size_t) p * ld;
    const int gi = ti * 16 + ar, gj = tj * 16 + ar;
    const bool ilive = gi < n, jlive = gj < n;
    const double mi = ilive ? mu[gi] : 0., mj = jlive ? mu[gj] : 0.;
    const int m0 = slab * AMALGAM_SLAB, m1 = min(c.ss, m0 + AMALGAM_SLAB);
    amalgam_d4 acc = { 0., 0., 0., 0. };
    for (int m = m0; m < m1; m += 4) {
        const int k = m + ak;
        const bool klive = k < m1;
        const double *x = d.X + (pb + ord[klive ? k : m0]) * ld;
        const double a = klive && ilive ? x[gi] - mi : 0.;
        const double b = klive && jlive ? x[gj] - mj : 0.;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    double *part = d.part + ((size_t) p * c.slabs + slab) * ld * ld;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = ti * 16 + ak + 4 * r;
        if (i < n && jlive) part[(size_t) i * ld + gj] = acc[r];
    }
}

// cov_ij <- (1 - etasigma) cov_ij + (etasigma / ss) (slab 0 + slab 1 + ...), j <= i, mirrored.
// grid (ceil(n n / 256), P), 256 threads
__global__ __launch_bounds__(256) void amalgam_cov(AmalgamDev d, AmalgamConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    if (pop_frozen(c, d.scal + p)) return;
    const int n = c.n, ld = c.ld, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * n) return;
    const int i = idx / n, j = idx % n;
    if (j > i) return;
    const size_t e = (size_t) i * ld + j, img = (size_t) ld * ld;
    const double *part = d.part + (size_t) p * c.slabs * img;
    double g = part[e];
    for (int s = 1; s < c.slabs; s++) g += part[s * img + e];
    double *cov = d.cov + (size_t) p * img;
    double v = cov[e] * (1. - c.etasigma);
    v += (c.etasigma / c.ss) * g;
    cov[e] = v;
    cov[(size_t) j * ld + i] = v;
}

// LINPACK's dchdc without pivoting (:455-528) on the upper triangle, right-looking, in panels of 16
// rows: inside a panel every step k takes the root of the pivot, scales row k and updates the rest of
// the panel's rows; then the panel's steps are applied to the trailing block, an entry at a time in
// the order of k -- the subtractions of an entry are the reference's, in its order.  A pivot <= 0
// ends the factorisation where it stands: the steps done so far are applied to everything, the rest
// is the Schur complement, no repair.  The result goes transposed into the lower triangle of chol,
// scaled by sqrt(cmult), the upper triangle zero (:406-415).  The matrix lives in LDS (ld <= 128) or
// in chol itself.  Every thread reads the pivot itself, so the decision to stop is the same in all of
// them without a flag, and a step costs two barriers: the root goes into the diagonal entry in the
// part that follows the scaling of row k, where nobody reads it.
// grid (P), 1024 threads (sixteen wavefronts hide the LDS round trips of the trailing update),
// LDS ld ld doubles or none
__global__ __launch_bounds__(1024) void amalgam_factor(AmalgamDev d, AmalgamConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    AmalgamScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, nt = blockDim.x, n = c.n, ld = c.ld;
    const double *cov = d.cov + (size_t) p * ld * ld;
    double *chol = d.chol + (size_t) p * ld * ld;
    double *A = c.lds_factor ? lds : chol;
    for (int idx = tid; idx < n * n; idx += nt) {
        const int i = idx / n, j = idx % n;
        A[(size_t) i * ld + j] = cov[(size_t) i * ld + j];
    }
    __syncthreads();
    int fail_at = n;
    for (int pb = 0; pb < n; pb += 16) {
        const int pe = min(pb + 16, n);
        int kdone = pe;
        for (int k = pb; k < pe; k++) {
            const double piv = A[(size_t) k * ld + k];
            if (piv <= 0.) {
                kdone = k;
                break;
            }
            const double t = sqrt(piv);
            for (int j = k + 1 + tid; j < n; j += nt) A[(size_t) k * ld + j] = A[(size_t) k * ld + j] / t;
            __syncthreads();
            if (tid == 0) A[(size_t) k * ld + k] = t;
            const int w = n - k - 1, rows = pe - k - 1;
            for (int idx = tid; idx < rows * w; idx += nt) {
                const int i = k + 1 + idx / w, j = k + 1 + idx % w;
                if (j < i) continue;
                A[(size_t) i * ld + j] = A[(size_t) i * ld + j] - A[(size_t) k * ld + j] * A[(size_t) k * ld + i];
            }
            __syncthreads();
        }
        const int w = n - pe;
        for (int idx = tid; idx < w * w; idx += nt) {
            const int i = pe + idx / w, j = pe + idx % w;
            if (j < i) continue;
            double v = A[(size_t) i * ld + j];
            for (int k = pb; k < kdone; k++) v = v - A[(size_t) k * ld + j] * A[(size_t) k * ld + i];
            A[(size_t) i * ld + j] = v;
        }
        __syncthreads();
        if (kdone < pe) {
            fail_at = kdone;
            break;
        }
    }
    const double s = sqrt(sc->cmult);
    for (int idx = tid; idx < n * n; idx += nt) {
        const int i = idx / n, j = idx % n;
        if (j > i) continue;
        const double v = A[(size_t) j * ld + i] * s;
        if (j < i) chol[(size_t) j * ld + i] = 0.;      // (in place: the pair (i, j) is this thread's alone)
        chol[(size_t) i * ld + j] = v;
    }
    if (tid == 0) {
        sc->fail_at = fail_at;
        if (fail_at < n) sc->fact_fail++;
    }
}

// The rows of Z: a wavefront per row, lane q takes the Philox call (row, q, generation, population)
// -- four ziggurat normals, columns 4 q .. 4 q + 3; amalgam_settle takes the slow path of the draws
// the fast test left open (a NaN marks them), with the seed read per lane (see hees_settle).
// grid (ceil(np / 4), P), 256 threads, both
__global__ __launch_bounds__(256) void amalgam_draw(AmalgamDev d, AmalgamConst c)
{
    const int p = blockIdx.y;
    const AmalgamScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave, n = c.n;
    if (r >= c.np) return;
    double *z = d.Z + ((size_t) p * c.np + r) * c.ld;
    const uint32_t gen = (uint32_t) sc->gen, sw = stream_word(STREAM_AMALGAM_NORMAL, amalgam_sub(c, p));
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

__global__ __launch_bounds__(256) void amalgam_settle(AmalgamDev d, AmalgamConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const AmalgamScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave, n = c.n;
    if (r >= c.np) return;
    double *z = d.Z + ((size_t) p * c.np + r) * c.ld;
    const uint32_t gen = (uint32_t) sc->gen, sw = stream_word(STREAM_AMALGAM_NORMAL, amalgam_sub(c, p));
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
__global__ __launch_bounds__(256) void amalgam_take(AmalgamDev d, AmalgamConst c)
{
    const int p = blockIdx.y;
    if (pop_frozen(c, d.scal + p)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave;
    if (r >= c.np) return;
    const size_t row = ((size_t) p * c.np + r) * c.ld;
    for (int j = lane; j < c.n; j += 64) d.Z[row + j] = d.zin[row + j];
}

// X = mu + Z chol^T on the fp64 matrix pipe: a workgroup per 16 rows, its wavefronts take every
// fourth tile of 16 coordinates.  The A operand is Z[row][l], the B operand chol[coordinate][l]; chol
// is lower triangular, so K ends with the tile's own diagonal block and the tiles of the zero
// triangle are never read.  Row 0 keeps the elite's x under keep_elite.
// grid (ceil(np / 16), P), 256 threads
__global__ __launch_bounds__(256) void amalgam_points(AmalgamDev d, AmalgamConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    if (pop_frozen(c, d.scal + p)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ar = lane & 15, ak = lane >> 4;
    const int n = c.n, ld = c.ld, np = c.np;
    const size_t pb = (size_t) p * np, pv = (size_t) p * ld;
    const double *chol = d.chol + (size_t) p * ld * ld;
    const int gm = blockIdx.x * 16 + ar;
    const bool mlive = gm < np;
    const double *zrow = d.Z + (pb + min(gm, np - 1)) * ld;
    for (int ct = wave; 16 * ct < n; ct += 4) {
        const int gi = ct * 16 + ar, kend = min(n, ct * 16 + 16);
        const bool ilive = gi < n;
        const double *lrow = chol + (size_t) min(gi, n - 1) * ld;
        amalgam_d4 acc = { 0., 0., 0., 0. };
        for (int l0 = 0; l0 < kend; l0 += 4) {
            const int l = l0 + ak;
            const double a = mlive && l < kend ? zrow[l] : 0.;
            const double b = ilive && l < kend ? lrow[l] : 0.;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = blockIdx.x * 16 + ak + 4 * r;
            if (m < np && ilive) {
                double x = d.mu[pv + gi] + acc[r];
                if (m == 0 && c.keep_elite) x = d.xelite[pv + gi];
                d.X[(pb + m) * ld + gi] = x;
            }
        }
    }
}

// The anticipated mean shift and the objective: a wavefront per row.  Of the rows 1 .. np - 1, nams
// take x += 2 cmult mushift: the rows a keyed shuffle of np - 1 slots sends below nams (cso_perm), or
// the rows the caller's table names.  Rows 1 .. are evaluated; row 0 keeps the elite's value next to
// its new x (:439-451).  grid (ceil(np / 4), P), 256 threads, LDS 4 ld doubles
__global__ __launch_bounds__(256) void amalgam_eval(AmalgamDev d, AmalgamConst c)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int p = blockIdx.y;
    const AmalgamScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave, n = c.n, ld = c.ld, np = c.np;
    if (r >= np) return;
    const size_t pb = (size_t) p * np, row = (pb + r) * ld, pv = (size_t) p * ld;
    int shift = 0;
    if (r > 0) {
        if (d.shin) shift = d.shin[pb + r];
        else shift = cso_perm((uint32_t) (r - 1), c.kb, (uint32_t) (np - 1), c.seed, (uint32_t) sc->gen,
                stream_word(STREAM_AMALGAM_SHIFT, amalgam_sub(c, p))) < (uint32_t) c.nams ? 1 : 0;
    }
    if (lane == 0) d.shifted[pb + r] = shift;
    if (r == 0) {
        if (lane == 0) d.f[pb] = sc->felite;
        return;
    }
    double *xl = lds + (size_t) wave * ld;
    const double a = 2. * sc->cmult;
    for (int j = lane; j < n; j += 64) {
        double x = d.X[row + j];
        if (shift) {
            x += a * d.mushift[pv + j];
            d.X[row + j] = x;
        }
        xl[j] = x;
    }
    wave_sync();
    if (c.obj < 0) return;      // a host objective evaluates X
    const double f = amalgam_objective(c, d, xl, lane);
    if (lane == 0) d.f[pb + r] = f;
}

// After the sampler, one workgroup per population (:213-233, :290-356):
//   any row better than row 0; their mean in row order minus mu, forward-substituted through the
//   scaled chol, max-norm = SDR; the rules of cmult and nis; the best ever evaluated; t, fev (np per
//   generation, as the reference counts); the stop tests: cmult < 1e-10, var(f) <= stol^2 over all np
//   stored values (the stale value of row 0 included), fev >= mfev.
// grid (P), 256 threads
__global__ __launch_bounds__(256) void amalgam_adapt(AmalgamDev d, AmalgamConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    AmalgamScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    __shared__ double stmp[AMALGAM_MAX_N], scratch[4], sval[4];
    __shared__ int sidx[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = c.n, ld = c.ld, np = c.np;
    const size_t pb = (size_t) p * np, pv = (size_t) p * ld;
    const double *f = d.f + pb, *chol = d.chol + (size_t) p * ld * ld;
    const double f0 = f[0], fbest0 = sc->fbest;
    double cnt = 0., fsum = 0., vmin = AMALGAM_INF;
    int imin = 0x7fffffff;
    for (int m = tid; m < np; m += 256) {
        const double fm = f[m];
        if (m > 0 && fm < f0) cnt += 1.;
        fsum += fm / np;
        if (fm < vmin) {
            vmin = fm;
            imin = m;
        }
    }
    const int count = (int) block_sum<4>(cnt, scratch);
    const double fmean = block_sum<4>(fsum, scratch);
    double vs = 0.;
    for (int m = tid; m < np; m += 256) {
        const double dv = f[m] - fmean;
        vs += dv * dv / np;
    }
    const double fvar = block_sum<4>(vs, scratch);
    block_arg<1>(vmin, imin, sval, sidx);
    const bool take = imin > 0 && imin < np && vmin < fbest0;
    if (take)
        for (int j = tid; j < n; j += 256) d.xbest[pv + j] = d.X[(pb + imin) * ld + j];
    double sdr = 0.;
    if (count > 0) {
        const double inv = 1. / count;
        for (int j = tid; j < n; j += 256) {
            double s = 0.;
            for (int m = 1; m < np; m++)
                if (f[m] < f0) s += d.X[(pb + m) * ld + j];
            s *= inv;
            s += -1. * d.mu[pv + j];
            stmp[j] = s;
        }
        __syncthreads();
        if (wave == 0) {
            for (int i = 0; i < n; i++) {
                const double *li = chol + (size_t) i * ld;
                double s = 0.;
                for (int l = lane; l < i; l += 64) s += li[l] * stmp[l];
                s = group_sum<64>(s);
                const double v = (stmp[i] - s) / li[i];
                wave_sync();
                if (lane == 0) stmp[i] = v;
                wave_sync();
                if (sdr < fabs(v)) sdr = fabs(v);
            }
        }
    }
    if (tid == 0) {
        double cm = sc->cmult;
        int nis = sc->nis;
        if (count > 0) {
            nis = 0;
            if (cm < 1.) cm = 1.;
            if (sdr > 1.) cm *= 1. / 0.9;
        } else {
            if (cm <= 1.) nis++;
            if (cm > 1. || nis >= c.nismax) cm *= 0.9;
            if (cm < 1. && nis < c.nismax) cm = 1.;
        }
        sc->cmult = cm;
        sc->nis = nis;
        sc->sdr = sdr;
        if (take) sc->fbest = vmin;
        sc->t++;
        sc->it++;
        sc->gen++;
        sc->fev += np;
        const bool own = cm < 1e-10 || fvar <= c.stol * c.stol, budget = sc->fev >= c.mfev;
        sc->conv = own || budget ? 1 : 0;
        if (!sc->stop) sc->stop = own ? 1 : budget ? 2 : 0;
    }
}

} // namespace bbo
