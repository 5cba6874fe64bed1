// bbo_chol_kernels.hpp -- the update of CholeskyCMAES (cholesky_cmaes.cpp) as gfx950 kernels.
//
//   kernel                 reference lines it replaces                         bound
//   chol_paths             cholesky_cmaes.cpp:56-77 (mean, dmean, pc),          latency (1 workgroup)
//                          :97-109 (forward substitution with the OLD A, ps)
//   chol_cprime            :79-95 as ONE matrix: C' = (1-c1-cmu) A A^T          fp64 MFMA (triangular SYRK
//                          + c1 pc pc^T + cmu sum w_i y_i y_i^T, lower tiles     + 2 n^2 flop / selected row)
//   chol_factor            :79-95,111-114 the factor the rank-1 chain ends with  fp64 MFMA trailing updates,
//                          = chol(C'); operand packing; updateSigma               serial panels (1 workgroup)
//   chol_history_stop      base_cmaes.cpp:191-209, :155, cholesky_cmaes.cpp:137-161  latency
//
// Why a factorisation: every rank-1 step of the reference keeps its matrix lower triangular with a
// positive diagonal, so what the mu + 1 steps leave is THE Cholesky factor of C' (unique).  The
// sampler takes A, packed in MFMA B-fragment order, where the dense variants pass B diag(D).
//
// Launch order within a generation: chol_paths and chol_cprime read the old factor, chol_factor
// writes the new one (and its packed form) after both -- one stream, no kernel reads a factor
// another is writing.  The old sigma serves all three; chol_factor's last act is updateSigma.
#pragma once

#include "bbo_cma_kernels.hpp"

namespace bbo {

// ---------------------------------------------------------------------------
// mean of the mu best (clamped), dmean, pc, w = A_old^-1 dmean, ps.  grid (P), 256 threads.
// Thread i owns row i of the substitution (and row i + 256 beyond n = 256): its part of A
// arrives 16 columns at a time ahead of the 16 steps that use it; a finished w_j goes round
// through LDS, one barrier per step.  Sums run in the reference's order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void chol_paths(CmaDev d, CmaConst c)
{
    const int p = blockIdx.x;
    CmaScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    __shared__ double wl[EIG_NMAX];
    __shared__ double red[4];
    const int tid = threadIdx.x, ld = c.ld, n = c.n;
    double *xmean = d.xmean + (size_t) p * ld, *xold = d.xold + (size_t) p * ld;
    double *ps = d.ps + (size_t) p * ld, *pc = d.pc + (size_t) p * ld;
    const double *A = d.A + (size_t) p * ld * ld;
    const double *X = d.X + (size_t) p * c.lambda_pad * ld;
    const int *order = d.order + (size_t) p * c.lambda_pad;
    const double sigma = sc->sigma;
    const double ccc = sqrt(c.cc * (2. - c.cc) * c.mueff);
    const double csc = sqrt(c.cs * (2. - c.cs) * c.mueff);

    double t[2] = { 0., 0. }, acc[2] = { 0., 0. };
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int j = tid + 256 * r;
        if (j >= ld) continue;
        const double xo = xmean[j];
        double xn = 0., pcj = 0.;
        if (j < n) {
            double sum = 0.;
            // (sixteen gathered rows requested before the first is added: the sum keeps the
            // reference's order, the loads do not wait for each other)
            int k = 0;
            for (; k + 16 <= c.mu; k += 16) {
                double xv[16], wv[16];
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    xv[u] = X[(size_t) order[k + u] * ld + j];
                    wv[u] = d.weights[k + u];
                }
#pragma unroll
                for (int u = 0; u < 16; u++) sum += wv[u] * xv[u];
            }
            for (; k < c.mu; k++) sum += d.weights[k] * X[(size_t) order[k] * ld + j];
            xn = sum;
            if (c.bound) xn = fmax(d.lower[j], fmin(xn, d.upper[j]));
            t[r] = (xn - xo) / sigma;
            pcj = (1. - c.cc) * pc[j] + ccc * t[r];
        }
        xold[j] = xo;
        xmean[j] = xn;
        pc[j] = pcj;
    }
    for (int jb = 0; jb < n; jb += 16) {
        double a[2][16];
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int i = tid + 256 * r;
#pragma unroll
            for (int k = 0; k < 16; k++) a[r][k] = (i < n && i >= jb) ? A[(size_t) i * ld + jb + k] : 0.;
        }
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int j = jb + k;
            if (j < n) {            // (uniform over the workgroup)
#pragma unroll
                for (int r = 0; r < 2; r++)
                    if (tid + 256 * r == j) {
                        t[r] = (t[r] - acc[r]) / a[r][k];
                        wl[j] = t[r];
                    }
                __syncthreads();
                const double wj = wl[j];
#pragma unroll
                for (int r = 0; r < 2; r++)
                    if (tid + 256 * r > j) acc[r] += a[r][k] * wj;
            }
        }
    }
    double ssq = 0.;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int j = tid + 256 * r;
        if (j >= ld) continue;
        const double v = j < n ? (1. - c.cs) * ps[j] + csc * t[r] : 0.;
        ps[j] = v;
        ssq += v * v;
    }
    ssq = group_sum<64>(ssq);
    if ((tid & 63) == 0) red[tid >> 6] = ssq;
    __syncthreads();
    if (tid == 0) sc->pslen = sqrt(red[0] + red[1] + red[2] + red[3]);
}

// ---------------------------------------------------------------------------
// C' on the matrix cores, one lower 16 x 16 tile per workgroup: grid (NT (NT + 1) / 2, P), 256
// threads.  C'(i, j) = sum_k coef_k v_k(i) v_k(j) over three families of vectors v_k:
//   the columns of A (coef 1 - c1 - cmu; A is lower triangular: only k < 16 (tj + 1) contribute),
//   the mu vectors y of the variant (coef cmu w_r): the first mu candidates about the NEW mean
//     (chol_paths ran first), or with `ranked` the mu best about the old one,
//   pc (coef c1).
// The four wavefronts take the k-steps round robin and are summed in a fixed order.
// Padding (i >= n): C' = I there, so the factor's padding is I too.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void chol_cprime(CmaDev d, CmaConst c)
{
    const int p = blockIdx.y;
    const CmaScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    __shared__ double part[4][256];
    int ti, tj;
    tri_tile(blockIdx.x, ti, tj);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ld = c.ld, n = c.n, ar = lane & 15, ak = lane >> 4;
    const int gi = ti * 16 + ar, gj = tj * 16 + ar;
    const double *A = d.A + (size_t) p * ld * ld;
    const double *X = d.X + (size_t) p * c.lambda_pad * ld;
    const int *order = d.order + (size_t) p * c.lambda_pad;
    const double *centre = (c.ranked ? d.xold : d.xmean) + (size_t) p * ld;
    const double *pc = d.pc + (size_t) p * ld;
    const double sigma = sc->sigma;
    const double ca = 1. - c.c1 - c.cmu;
    const int S1 = 4 * (tj + 1), S2 = (c.mu + 3) >> 2, S = S1 + S2 + 1;
    const double ci = gi < n ? centre[gi] : 0., cj = gj < n ? centre[gj] : 0.;

    d4_t acc = { 0., 0., 0., 0. };
    for (int s = wave; s < S; s += 4) {
        double a = 0., b = 0.;
        if (s < S1) {
            const int k = 4 * s + ak;
            a = ca * A[(size_t) gi * ld + k];
            b = A[(size_t) gj * ld + k];
        } else if (s < S1 + S2) {
            const int r = 4 * (s - S1) + ak;
            if (r < c.mu) {
                const size_t row = c.ranked ? order[r] : r;
                const double yi = gi < n ? (X[row * ld + gi] - ci) / sigma : 0.;
                const double yj = gj < n ? (X[row * ld + gj] - cj) / sigma : 0.;
                a = (c.cmu * d.weights[r]) * yi;
                b = yj;
            }
        } else if (ak == 0) {
            a = c.c1 * pc[gi];
            b = pc[gj];
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) part[wave][r * 64 + lane] = acc[r];
    __syncthreads();
    if (wave == 0) {
        double *C = d.C + (size_t) p * ld * ld;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int q = r * 64 + lane;
            double v = ((part[0][q] + part[1][q]) + part[2][q]) + part[3][q];
            const int i = ti * 16 + ak + 4 * r, j = tj * 16 + ar;
            if (i >= n || j >= n) v = (i == j) ? 1. : 0.;
            C[(size_t) i * ld + j] = v;
        }
    }
}

// ---------------------------------------------------------------------------
// A <- chol(C'), right-looking, 16-wide panels: grid (P), 256 threads.  The matrix sits in LDS
// (ld <= 128: rows of ld + 1 doubles) or stays in its global image (ld > 128: one workgroup per
// population walks it through L2).  Per panel: the 16 x 16 diagonal block unblocked on one
// wavefront, the rows below it solved against it one thread per row, the trailing tiles updated
// with four MFMAs each.  A pivot that rounding left non-positive is set to a tiny multiple of
// its original diagonal entry (kept aside in LDS) and counted (sticky, bbo_get "chol_repairs").
// Then: A (upper triangle and padding exactly 0) and its packed form for the sampler, and
// updateSigma (base_cmaes.cpp:176-189).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void chol_factor(CmaDev d, CmaConst c, int in_lds)
{
    const int p = blockIdx.x;
    CmaScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    extern __shared__ double chol_lds[];
    __shared__ int repairs;
    __shared__ double diag0[EIG_NMAX];      // the diagonal of C' as it came: the scale of a repaired pivot
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ld = c.ld, n = c.n, NT = ld >> 4;
    double *Cg = d.C + (size_t) p * ld * ld;
    double *M = in_lds ? chol_lds : Cg;
    const int lm = in_lds ? ld + 1 : ld;
    if (tid == 0) repairs = 0;
    for (int i = tid; i < ld; i += 256) diag0[i] = Cg[(size_t) i * ld + i];
    if (in_lds)
        for (int q = tid; q < ld * ld; q += 256) {
            const int i = q / ld, j = q - i * ld;
            if ((j >> 4) <= (i >> 4)) M[i * lm + j] = Cg[q];
        }
    __syncthreads();

    for (int kb = 0; kb < NT; kb++) {
        const int k0 = kb * 16;
        if (wave == 0) {
            const int r = lane;             // lanes 0..15: one row of the block each
            for (int j = 0; j < 16; j++) {
                double djj = M[(k0 + j) * lm + k0 + j];
                if (!(djj > 0.)) {
                    djj = 0x1p-52 * fmax(fabs(diag0[k0 + j]), 0x1p-900);
                    if (lane == 0) repairs++;
                }
                const double ljj = sqrt(djj);
                double l = 0.;
                if (r > j && r < 16) {
                    l = M[(k0 + r) * lm + k0 + j] / ljj;
                    M[(k0 + r) * lm + k0 + j] = l;
                }
                if (r == j) M[(k0 + j) * lm + k0 + j] = ljj;
                wave_sync();
                if (r > j && r < 16)
                    for (int k = j + 1; k <= r; k++)
                        M[(k0 + r) * lm + k0 + k] -= l * M[(k0 + k) * lm + k0 + j];
                wave_sync();
            }
        }
        __syncthreads();
        // rows below the block: L_ik = (M_ik - sum_q L_iq L_kq) / L_kk
        for (int i = k0 + 16 + tid; i < ld; i += 256) {
            double x[16];
#pragma unroll
            for (int j = 0; j < 16; j++) {
                double s = M[i * lm + k0 + j];
#pragma unroll
                for (int q = 0; q < j; q++) s -= x[q] * M[(k0 + j) * lm + k0 + q];
                x[j] = s / M[(k0 + j) * lm + k0 + j];
            }
#pragma unroll
            for (int j = 0; j < 16; j++) M[i * lm + k0 + j] = x[j];
        }
        __syncthreads();
        // trailing tiles (ti >= tj > kb): M -= L[ti, kb] L[tj, kb]^T
        const int rem = NT - kb - 1, tiles = rem * (rem + 1) / 2;
        const int ar = lane & 15, ak = lane >> 4;
        for (int q = wave; q < tiles; q += 4) {
            int ti, tj;
            tri_tile(q, ti, tj);
            ti += kb + 1;
            tj += kb + 1;
            d4_t acc;
#pragma unroll
            for (int r = 0; r < 4; r++) acc[r] = M[(ti * 16 + ak + 4 * r) * lm + tj * 16 + ar];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const double a = -M[(ti * 16 + ar) * lm + k0 + 4 * u + ak];
                const double b = M[(tj * 16 + ar) * lm + k0 + 4 * u + ak];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; r++) M[(ti * 16 + ak + 4 * r) * lm + tj * 16 + ar] = acc[r];
        }
        __syncthreads();
    }

    // the factor, row-major and packed: element (i, j) of the sampler's operand sits at tile i >> 4,
    // k-step j >> 2, lane (j & 3, i & 15)
    double *Ag = d.A + (size_t) p * ld * ld, *pk = d.BDp + (size_t) p * ld * ld;
    const int KS = ld >> 2;
    for (int q = tid; q < ld * ld; q += 256) {
        const int i = q / ld, j = q - i * ld;
        const double v = (j <= i && i < n) ? M[i * lm + j] : 0.;
        pk[((size_t) (i >> 4) * KS + (j >> 2)) * 64 + ((j & 3) << 4) + (i & 15)] = v;
    }
    for (int q = tid; q < ld * ld; q += 256) {
        const int i = q / ld, j = q - i * ld;
        Ag[q] = (j <= i && i < n) ? M[i * lm + j] : 0.;
    }
    if (tid == 0) {
        const double *f = d.f + (size_t) p * c.lambda_pad;
        const int *order = d.order + (size_t) p * c.lambda_pad;
        double sg = sc->sigma * exp(fmin(1., (c.cs / c.damps) * (sc->pslen / c.chi - 1.)));
        if (f[order[0]] == f[order[c.ik]]) sg *= exp(0.2 + c.cs / c.damps);
        if (sc->it >= c.hlen && sc->fworst - sc->fbest == 0.) sg *= exp(0.2 + c.cs / c.damps);
        sc->sigma = sg;
        d.chol_repairs[p] += repairs;
    }
}

// ---------------------------------------------------------------------------
// updateHistory, it++, CholeskyCmaes::converged (its own two-part rule, flag 11), budget.
// grid (P), 256 threads.  The radii ||x_k|| are only formed when the fitness part holds
// (16 lanes per candidate; mean and squared deviations in two passes over d.zn2 as scratch).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void chol_history_stop(CmaDev d, CmaConst c)
{
    const int p = blockIdx.x;
    CmaScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, ld = c.ld;
    double *hb = d.hist_best + (size_t) p * c.hlen, *hk = d.hist_kth + (size_t) p * c.hlen;
    const double *f = d.f + (size_t) p * c.lambda_pad;
    const int *order = d.order + (size_t) p * c.lambda_pad;
    int it = sc->it, head = sc->hist_head, len = sc->hist_len;
    double fbest = sc->fbest, fworst = sc->fworst;
    if (it < c.mit) {
        head = (head + 1) % c.hlen;
        if (len < c.hlen) len++;
        if (tid < 64) {
            if (lane == 0) {
                hb[head] = f[order[0]];
                hk[head] = f[order[c.ik]];
            }
            wave_sync();
            if (len == c.hlen) {
                double lo = BBO_INF, hi = -BBO_INF;
                for (int k = lane; k < c.hlen; k += 64) {
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
    }
    it++;
    int flag = 0;
    if (fabs(f[order[0]] - f[order[c.lambda - 1]]) <= c.tol) {      // (uniform over the workgroup)
        double *rad = d.zn2 + (size_t) p * c.lambda_pad;
        const double *X = d.X + (size_t) p * c.lambda_pad * ld;
        const int g = tid & 15;
        for (int k = tid >> 4; k < c.lambda; k += 16) {
            double s = 0.;
            for (int j = g; j < c.n; j += 16) s += X[(size_t) k * ld + j] * X[(size_t) k * ld + j];
            s += __shfl_xor(s, 8, 64);
            s += __shfl_xor(s, 4, 64);
            s += __shfl_xor(s, 2, 64);
            s += __shfl_xor(s, 1, 64);
            if (g == 0) rad[k] = sqrt(s);
        }
        __syncthreads();
        double s = 0.;
        for (int k = tid; k < c.lambda; k += 256) s += rad[k];
        s = group_sum<64>(s);
        if (lane == 0) red[tid >> 6] = s;
        __syncthreads();
        const double mean = (((red[0] + red[1]) + red[2]) + red[3]) / c.lambda;
        __syncthreads();
        s = 0.;
        for (int k = tid; k < c.lambda; k += 256) s += (rad[k] - mean) * (rad[k] - mean);
        s = group_sum<64>(s);
        if (lane == 0) red[tid >> 6] = s;
        __syncthreads();
        const double m2 = ((red[0] + red[1]) + red[2]) + red[3];
        if (m2 <= (c.lambda - 1) * c.stol * c.stol) flag = 11;
    }
    if (tid == 0) {
        sc->it = it;
        sc->hist_head = head;
        sc->hist_len = len;
        sc->fbest = fbest;
        sc->fworst = fworst;
        sc->flag = flag;
        if (flag) sc->stop = 1;
        else if (sc->fev >= c.mfev) sc->stop = 2;
    }
}

} // namespace bbo
