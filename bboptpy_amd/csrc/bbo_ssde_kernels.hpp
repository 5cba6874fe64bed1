// bbo_ssde_kernels.hpp -- SSDE as gfx950 kernels.
//
//   kernel            reference lines (ssde.cpp)                                   work per population
//   ssde_init         :87-131 the pool, its opposites, their values, the sort,     npinit or 2 npinit rows
//                     the memory
//   ssde_generation   :134-361 one iterate(): randA, the np member steps, the      np .. 2 np evaluations
//                     memory update, the sort, the shrink, and converged()
//                     (:383-408); or, entered and left at an evaluation, the
//                     part of it up to the next one
//   ssde_eval         the value of the pending point                               one row
#pragma once

#include "bbo_ssde.hpp"
#include "bbo_objectives.hpp"
#include "bbo_rng.hpp"
#include "bbo_wave.hpp"
#include "bbo_rank.hpp"

namespace bbo {

#define SSDE_INF (__builtin_huge_val())

// std::sin(1e-12) and std::cos(1e-12) (:427-429): x - x^3 / 6 and 1 - x^2 / 2 round to x and to 1
#define SSDE_SIN 1e-12
#define SSDE_COS 1.

enum SsdeInitMode { SSDE_INIT_DRAW = 1, SSDE_INIT_OPP = 2, SSDE_INIT_EVAL = 4, SSDE_INIT_RESET = 8, SSDE_INIT_SORT = 16 };

// what a coordinate is in the generation's matrix A
enum SsdeRole { SSDE_ALONE = 0, SSDE_FIRST, SSDE_SECOND };

// Random::get(a, b) of the reference on doubles (random.hpp:329-337) over the raw uniform u
__device__ inline double ssde_between(double u, double a, double b)
{
#pragma clang fp contract(off)
    const double lo = a < b ? a : b, hi = a < b ? b : a;
    return u * (hi - lo) + lo;
}

// The draws of one population in one generation.  The table of bbo_ssde_inject_draws and of
// "record_draws": [perm: n][npinit x (9 + 3 n)], per member the outcomes iL, zr, p, q, r, pbest, ci, zcr,
// j0, then the uniforms of b, of the crossover and of the redraw.  The generator's counters name what a
// draw is for -- (coordinate | purpose, member | attempt, generation) -- never when it is made: how many
// draws another member took does not move a later one.
struct SsdeDraws {
    const double *inj;
    double *rec;
    uint64_t seed;
    uint32_t sub, gen;
    int n;

    __device__ size_t member(int i) const { return (size_t) n + (size_t) i * (SSDE_REC_HEAD + 3 * (size_t) n); }

    __device__ u32x4 word(int purpose, int i, int attempt) const
    {
        return philox4x32_10_uniform(seed, (uint32_t) purpose << 16, (uint32_t) i | ((uint32_t) attempt << 16), gen,
                stream_word(STREAM_SSDE_CTRL, sub));
    }
    // one index of sample3 (:459-472): at most SSDE_MAX_TRIES draws, then the next free index cyclically
    __device__ int distinct(int purpose, int i, int np, int a, int b, int c) const
    {
        int v = 0;
        for (int t = 0; t < SSDE_MAX_TRIES; t++) {
            v = uint_below(word(purpose, i, t).x, np);
            if (v != a && v != b && v != c) return v;
        }
        for (int t = 0; t < 4; t++) {
            v = v + 1 < np ? v + 1 : 0;
            if (v != a && v != b && v != c) break;
        }
        return v;
    }
    // the draws of member i up to its spherical trial (:151-170, :225-229), by ONE thread
    __device__ void ctrl(int i, int np, int H, int itop, const double *L2, int &iL, double &zr, int &p, int &q,
            int &r, int &pbest, double &ci) const
    {
        const size_t o = member(i);
        if (inj) {
            iL = min(max((int) inj[o], 0), H - 1);
            zr = inj[o + 1];
            p = min(max((int) inj[o + 2], 0), np - 1);
            q = min(max((int) inj[o + 3], 0), np - 1);
            r = min(max((int) inj[o + 4], 0), np - 1);
            pbest = min(max((int) inj[o + 5], 0), np - 1);
            ci = inj[o + 6];
        } else {
            const u32x4 w = word(0, i, 0);
            iL = uint_below(w.x, H);
            pbest = uint_below(w.y, itop + 1);
            double z1, z2, z3;
            normal_quad(seed, 6u << 16, (uint32_t) i, gen, stream_word(STREAM_SSDE_CTRL, sub), zig_global_wk(), zr, z1,
                    z2, z3);
            p = distinct(1, i, np, i, -1, -1);
            q = distinct(2, i, np, i, p, -1);
            r = distinct(3, i, np, i, p, q);
            // :225-229 the Cauchy step: at most SSDE_MAX_TRIES draws, then min(1, L2[iL])
            const double l2 = L2[iL];
            ci = l2;
            for (int t = 0; t < SSDE_MAX_TRIES; t++) {
                const u32x4 wc = word(4, i, t);
                const double cand = tan(M_PI * (u01(wc.x, wc.y) - 0.5)) * 0.1 + l2;
                if (cand > 0.) {
                    ci = cand;
                    break;
                }
            }
            ci = ci < 1. ? ci : 1.;
        }
        if (rec) {
            rec[o] = iL;
            rec[o + 1] = zr;
            rec[o + 2] = p;
            rec[o + 3] = q;
            rec[o + 4] = r;
            rec[o + 5] = pbest;
            rec[o + 6] = ci;
        }
    }
    // the draws of the DE trial that all lanes share (:253-258), by ONE thread
    __device__ void ctrl_de(int i, double &zcr, int &j0) const
    {
        const size_t o = member(i);
        if (inj) {
            zcr = inj[o + 7];
            j0 = min(max((int) inj[o + 8], 0), n - 1);
        } else {
            double z0, z2, z3;
            normal_quad(seed, 6u << 16, (uint32_t) i, gen, stream_word(STREAM_SSDE_CTRL, sub), zig_global_wk(), z0, zcr,
                    z2, z3);
            j0 = uint_below(word(5, i, 0).x, n);
        }
        if (rec) {
            rec[o + 7] = zcr;
            rec[o + 8] = j0;
        }
    }
    // the uniform of b[dd] (:157)
    __device__ double ub(int i, int dd, bool keep) const
    {
        const size_t o = member(i) + SSDE_REC_HEAD + (size_t) dd;
        double u;
        if (inj) u = inj[o];
        else {
            const u32x4 w = philox4x32_10(seed, (uint32_t) dd, (uint32_t) i, gen, stream_word(STREAM_SSDE_R, sub));
            u = u01(w.x, w.y);
        }
        if (rec && keep) rec[o] = u;
        return u;
    }
    // the uniforms of the crossover (:260) and of the redraw inside the box (:265)
    __device__ double ucross(int i, int dd) const
    {
        const size_t o = member(i) + SSDE_REC_HEAD + (size_t) n + (size_t) dd;
        double u;
        if (inj) u = inj[o];
        else {
            const u32x4 w = philox4x32_10(seed, (uint32_t) dd, (uint32_t) i, gen, stream_word(STREAM_SSDE_R, sub));
            u = u01(w.z, w.w);
        }
        if (rec) rec[o] = u;
        return u;
    }
    __device__ double uredraw(int i, int dd) const
    {
        const size_t o = member(i) + SSDE_REC_HEAD + 2 * (size_t) n + (size_t) dd;
        double u;
        if (inj) u = inj[o];
        else {
            const u32x4 w = philox4x32_10(seed, (uint32_t) dd | (1u << 16), (uint32_t) i, gen,
                    stream_word(STREAM_SSDE_R, sub));
            u = u01(w.x, w.y);
        }
        if (rec) rec[o] = u;
        return u;
    }
};

// dnrm2 of the reference (blas.cpp:154-181), one thread
__device__ inline double ssde_dnrm2(int n, const double *x)
{
#pragma clang fp contract(off)
    if (n == 1) return fabs(x[0]);
    double scale = 0., ssq = 1.;
    for (int i = 0; i < n; i++) {
        const double v = x[i];
        if (v != 0.) {
            const double a = fabs(v);
            if (scale < a) {
                ssq = 1. + ssq * (scale / a) * (scale / a);
                scale = a;
            } else {
                ssq = ssq + (a / scale) * (a / scale);
            }
        }
    }
    return scale * sqrt(ssq);
}

// the first test of converged() (:386-401) over the norms in rank order, one thread
__device__ inline int ssde_spread_converged(const double *radius, int np, double tol)
{
#pragma clang fp contract(off)
    int count = 0;
    double mean = 0., m2 = 0.;
    for (int k = 0; k < np; k++) {
        const double x = radius[k];
        count++;
        const double delta = x - mean;
        mean += delta / count;
        const double delta2 = x - mean;
        m2 += delta * delta2;
    }
    return m2 <= (np - 1) * tol * tol ? 1 : 0;
}

// std::sort by fitness (:115, :345) of the ranks [0, count): the row of rank k goes to the place that
// pair_less (fitness, then the rank it had) gives it, so ties keep their order.  dst and src differ.
template<int T>
__device__ inline void ssde_sort(const double *gf, const int *src, int *dst, int count, int tid)
{
    for (int k = tid; k < count; k += T) {
        const int row = src[k];
        const double fk = gf[row];
        int place = 0;
        for (int j = 0; j < count; j++) place += pair_less(gf[src[j]], j, fk, k) ? 1 : 0;
        dst[place] = row;
    }
}

// :87-131 for the populations p0 .. p0 + gridDim.x - 1; also what follows a set of "x".  DRAW: npinit
// uniform rows; OPP: their opposites behind them; EVAL: the values of the rows [r0, r1), a wavefront per
// row; RESET: the memory and the counters, fev = r1; SORT: the rows [0, r1) ranked, np = min(r1, npinit),
// the norms and converged().  grid (populations), 256 threads
__global__ __launch_bounds__(256) void ssde_init(SsdeDev d, SsdeConst c, int p0, int mode, int r0, int r1)
{
#pragma clang fp contract(off)
    const int p = p0 + blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int n = c.n, ld = c.ld, npinit = c.npinit;
    const size_t pr = (size_t) p * c.nrows;
    double *gx = d.x + pr * ld, *gf = d.f + pr;
    int *ord = d.order + pr, *ord2 = d.order2 + pr;
    const uint32_t sub = (uint32_t) (c.sub0 + p);
    if (mode & SSDE_INIT_DRAW) {
        for (int r = wave; r < npinit; r += 4)
            for (int j = lane; j < n; j += 64) {
                const u32x4 w = philox4x32_10(c.seed, (uint32_t) r, (uint32_t) j, 0, stream_word(STREAM_SSDE_INIT, sub));
                gx[(size_t) r * ld + j] = ssde_between(u01(w.x, w.y), d.lower[j], d.upper[j]);
            }
        __syncthreads();
    }
    if ((mode & SSDE_INIT_OPP) && c.nrows >= 2 * npinit) {
        for (int r = wave; r < npinit; r += 4)
            for (int j = lane; j < n; j += 64)
                gx[(size_t) (npinit + r) * ld + j] = d.lower[j] + d.upper[j] - gx[(size_t) r * ld + j];
        __syncthreads();
    }
    if (mode & SSDE_INIT_EVAL) {
        for (int r = r0 + wave; r < r1; r += 4) {
            double f = eval_row_group<64>(c.obj, n, gx + (size_t) r * ld, d.aux, lane);
            if (f != f) f = SSDE_INF;
            if (lane == 0) gf[r] = f;
        }
        __syncthreads();
    }
    if (mode & SSDE_INIT_RESET) {
        for (int k = tid; k < c.H; k += 256) {
            d.L1[(size_t) p * c.H + k] = 0.5;
            d.L2[(size_t) p * c.H + k] = 0.5;
            d.LCR[(size_t) p * c.H + k] = 0.5;
        }
        for (int j = tid; j < ld; j += 256) {
            d.perm[(size_t) p * ld + j] = j < n ? j : 0;
            d.cand[(size_t) p * ld + j] = 0.;
        }
        __syncthreads();
    }
    if (mode & SSDE_INIT_SORT) {
        // (the rows in place are ranked from the identity: ties in row order)
        for (int k = tid; k < c.nrows; k += 256) ord2[k] = k;
        __syncthreads();
        ssde_sort<256>(gf, ord2, ord, r1, tid);
        for (int k = r1 + tid; k < c.nrows; k += 256) ord[k] = k;
        __syncthreads();
        const int np = r1 < npinit ? r1 : npinit;
        for (int k = tid; k < np; k += 256) d.radius[(size_t) p * npinit + k] = ssde_dnrm2(n, gx + (size_t) ord[k] * ld);
        __syncthreads();
    }
    if (tid == 0 && (mode & (SSDE_INIT_RESET | SSDE_INIT_SORT))) {
        SsdeScal s = d.scal[p];
        if (mode & SSDE_INIT_RESET) {
            s = SsdeScal {};
            s.fev = r1;
            s.k = s.kCR = 1;
            d.fcand[p] = 0.;
        }
        if (mode & SSDE_INIT_SORT) {
            s.np = r1 < npinit ? r1 : npinit;
            s.oldbestf = gf[ord[0]];
            s.conv = ssde_spread_converged(d.radius + (size_t) p * npinit, s.np, c.tol) || s.convcount > c.patience
                    ? 1 : 0;
            s.stage = SSDE_IDLE;
            s.pending = 0;
            s.lenS = s.lenSCR = 0;
        }
        d.scal[p] = s;
    }
}

// the value of the pending point.  grid (P), 64 threads
__global__ __launch_bounds__(64) void ssde_eval(SsdeDev d, SsdeConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    if (pop_frozen(c, d.scal + p) || !d.scal[p].pending) return;
    double f = eval_row_group<64>(c.obj, c.n, d.cand + (size_t) p * c.ld, d.aux, threadIdx.x);
    if (f != f) f = SSDE_INF;
    if (threadIdx.x == 0) d.fcand[p] = f;
}

// the hand-over point of the workgroup's T threads
template<int T>
__device__ inline void ssde_sync()
{
    if (T == 64) wave_sync();
    else __syncthreads();
}

// One iterate() of the reference per launch (mode SSDE_FUSED), or the piece of it between two evaluations
// (SSDE_ADVANCE, SSDE_ABSORB): the same body, a state machine over SsdeStage whose position lives in the
// population's scalars between launches, so the two paths run the same instructions on the same values.
// One workgroup of T threads per population.  The lanes own the coordinates (z, the two sparse passes of
// A, the DE point, the copies); thread 0 draws what the lanes share and keeps the generation's successes
// in global memory; the first wavefront sums the objective from LDS with eval_row_group<64>.
// The matrix of the generation lives as two arrays: partner[d] and role[d].  With s = sin(1e-12) and
// c = cos(1e-12), a pair (a, b) = (perm[2 i], perm[2 i + 1]) has A[a][a] = A[b][b] = s, A[a][b] = c,
// A[b][a] = -c; a leftover coordinate has A[d][d] = 1.  The two terms of a row of A z, and of a column of
// A' work added onto x[d], enter in the order of their index, as the dense loops add them.  The dense
// loops' other terms are products with 0.: they change nothing while z is finite, and where it is not the
// reference's 0 * inf poisons the whole row, which this kernel does not reproduce.
// `begin`: an idle population starts its next generation (the first SSDE_ADVANCE of a generation).
// LDS: lower, upper, z, work, row [ld] each, partner and role [ld] ints.
// grid (P), T threads
template<int T>
__global__ __launch_bounds__(T) void ssde_generation(SsdeDev d, SsdeConst c, int mode, int begin)
{
#pragma clang fp contract(off)
    constexpr int W = T / 64;
    extern __shared__ double ssde_lds[];
    __shared__ double bc_f[4];
    __shared__ int bc_i[8];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = c.n, ld = c.ld, npinit = c.npinit, H = c.H;
    SsdeScal s = d.scal[p];
    if (pop_frozen(c, &s)) return;
    if (mode == SSDE_ABSORB && !s.pending) return;
    if (mode == SSDE_ADVANCE && s.pending) return;      // (a value is still owed)
    // (a population that has completed its generation waits for the others of the handle)
    if (mode == SSDE_ADVANCE && s.stage == SSDE_IDLE && !begin) return;
    const size_t pr = (size_t) p * c.nrows, pm = (size_t) p * npinit;
    double *gx = d.x + pr * ld, *gf = d.f + pr;
    int *ord = d.order + pr, *gperm = d.perm + (size_t) p * ld;
    double *L1 = d.L1 + (size_t) p * H, *L2 = d.L2 + (size_t) p * H, *LCR = d.LCR + (size_t) p * H;
    double *lo = ssde_lds, *up = lo + ld, *z = up + ld, *work = z + ld, *row = work + ld;
    int *partner = reinterpret_cast<int*>(row + ld), *role = partner + ld;
    const size_t tlen = (size_t) n + (size_t) npinit * (SSDE_REC_HEAD + 3 * (size_t) n);
    const SsdeDraws q { d.inject ? d.inject + (size_t) p * tlen : nullptr, d.draws ? d.draws + (size_t) p * tlen : nullptr,
            c.seed, (uint32_t) (c.sub0 + p), (uint32_t) s.gen, n };

    // partner and role from the permutation in global memory
    auto build_pairs = [&]() {
        for (int pos = tid; pos < n; pos += T) {
            const int dd = gperm[pos];
            if ((n & 1) && pos == n - 1) {
                partner[dd] = dd;
                role[dd] = SSDE_ALONE;
            } else if (!(pos & 1)) {
                partner[dd] = gperm[pos + 1];
                role[dd] = SSDE_FIRST;
            } else {
                partner[dd] = gperm[pos - 1];
                role[dd] = SSDE_SECOND;
            }
        }
        ssde_sync<T>();
    };
    // the value of a row in LDS, in every thread
    auto evaluate = [&](const double *r) {
        double f = 0.;
        if (wave == 0) {
            f = eval_row_group<64>(c.obj, n, r, d.aux, lane);
            if (f != f) f = SSDE_INF;
            if (W > 1 && lane == 0) bc_f[3] = f;
        }
        if (W > 1) {
            __syncthreads();
            f = bc_f[3];
            __syncthreads();
        }
        return f;
    };
    // the trial in `row` becomes the pending point
    auto publish = [&]() {
        for (int i = tid; i < n; i += T) d.cand[(size_t) p * ld + i] = row[i];
        s.pending = 1;
    };
    // :237-248, :281-292 the value f of the trial in `row` against member mi: <= replaces, < is a success
    auto select = [&](double f, bool &better) {
        const int rowi = ord[s.mi];
        const double fi = gf[rowi];
        ssde_sync<T>();
        better = f < fi;
        if (!(f <= fi)) return false;
        if (tid == 0) gf[rowi] = f;
        for (int i = tid; i < n; i += T) gx[(size_t) rowi * ld + i] = row[i];
        ssde_sync<T>();
        return true;
    };

    if (mode == SSDE_FUSED) s.pending = 0;
    for (int i = tid; i < n; i += T) {
        lo[i] = d.lower[i];
        up[i] = d.upper[i];
        if (s.stage == SSDE_WAIT_SS || s.stage == SSDE_WAIT_DE) row[i] = d.cand[(size_t) p * ld + i];
    }
    ssde_sync<T>();
    if (s.stage != SSDE_IDLE) build_pairs();

    for (;;) {
        if (s.stage == SSDE_IDLE) {
            if (mode == SSDE_ABSORB) break;
            // randA (:410-432): a fresh uniform permutation, its consecutive pairs the rotated planes
            if (q.rec) {
                for (size_t e = tid; e < tlen; e += T) q.rec[e] = 0.;
                ssde_sync<T>();
            }
            if (q.inj) {
                for (int pos = tid; pos < n; pos += T) gperm[pos] = min(max((int) q.inj[pos], 0), n - 1);
            } else if (!s.keep_perm && n > 1) {
                int kb = 1;
                while ((1u << kb) < (unsigned) n) kb++;
                kb = (kb + 1) / 2;
                for (int pos = tid; pos < n; pos += T)
                    gperm[pos] = (int) cso_perm((uint32_t) pos, kb, (uint32_t) n, c.seed, (uint32_t) s.gen,
                            stream_word(STREAM_SSDE_PERM, q.sub));
            }
            s.keep_perm = 0;
            ssde_sync<T>();
            if (q.rec)
                for (int pos = tid; pos < n; pos += T) q.rec[pos] = gperm[pos];
            build_pairs();
            s.oldbestf = gf[ord[0]];
            s.lenS = s.lenSCR = 0;
            s.mi = 0;
            s.stage = SSDE_MEMBER;
        }
        if (s.stage == SSDE_MEMBER) {
            if (s.mi >= s.np) {
                // :296-342 the memory: the weighted Lehmer means of the successes, in member order
                if (tid == 0) {
                    if (s.lenS > 0) {
                        double rnum = 0., rden = 0., cnum = 0., cden = 0.;
                        for (int i = 0; i < s.lenS; i++) {
                            const double w = d.w[pm + i], sr = d.SR[pm + i], sc = d.SC[pm + i];
                            rnum += w * sr * sr;
                            rden += w * sr;
                            cnum += w * sc * sc;
                            cden += w * sc;
                        }
                        L1[s.k - 1] = rnum / rden;
                        L2[s.k - 1] = cnum / cden;
                    }
                    if (c.usede && s.lenSCR > 0) {
                        double num = 0., den = 0.;
                        for (int i = 0; i < s.lenSCR; i++) {
                            const double w = d.wCR[pm + i], cr = d.SCR[pm + i];
                            num += w * cr * cr;
                            den += w * cr;
                        }
                        LCR[s.kCR - 1] = num / den;
                    }
                }
                if (s.lenS > 0 && ++s.k > H) s.k = 1;
                if (c.usede && s.lenSCR > 0 && ++s.kCR > H) s.kCR = 1;
                // :345 the sort, :348-352 convcount, :355-360 the shrink (never under SSDE_MIN_NP)
                int *ord2 = d.order2 + pr;
                ssde_sort<T>(gf, ord, ord2, s.np, tid);
                ssde_sync<T>();
                for (int k = tid; k < s.np; k += T) ord[k] = ord2[k];
                ssde_sync<T>();
                if (gf[ord[0]] < s.oldbestf) s.convcount = 0;
                else s.convcount++;
                const int npnew = (int) (npinit + (c.npmin - npinit) * (1. * s.fev) / c.mfev);
                if (s.np > npnew) s.np = npnew > SSDE_MIN_NP ? npnew : SSDE_MIN_NP;
                // converged() (:383-408)
                for (int k = tid; k < s.np; k += T) d.radius[pm + k] = ssde_dnrm2(n, gx + (size_t) ord[k] * ld);
                ssde_sync<T>();
                if (tid == 0) bc_i[0] = ssde_spread_converged(d.radius + pm, s.np, c.tol);
                ssde_sync<T>();
                s.conv = bc_i[0] || s.convcount > c.patience ? 1 : 0;
                if (s.conv) s.stop = 1;
                else if (s.fev >= c.mfev) s.stop = 2;
                s.gen++;
                s.stage = SSDE_IDLE;
                s.pending = 0;
                break;
            }
            // :151-170 the shared draws, :173 R, :225-229 the step
            const int itop = max(1, (int) (c.ptop * s.np));
            if (tid == 0) {
                int iL, pi, qi, ri, pbest;
                double zr, ci;
                q.ctrl(s.mi, s.np, H, itop, L2, iL, zr, pi, qi, ri, pbest, ci);
                double prank = zr * 0.1 + L1[iL];
                prank = prank < 1. ? prank : 1.;        // std::min(1., .), then std::max(0., .)
                prank = 0. < prank ? prank : 0.;
                bc_i[0] = iL;
                bc_i[1] = pi;
                bc_i[2] = qi;
                bc_i[3] = ri;
                bc_i[4] = pbest;
                bc_f[0] = prank;
                bc_f[1] = ci;
            }
            ssde_sync<T>();
            s.iL = bc_i[0];
            s.pi = bc_i[1];
            s.qi = bc_i[2];
            s.ri = bc_i[3];
            const int pbest = bc_i[4];
            s.prank = bc_f[0];
            s.ci = bc_f[1];
            s.R = (1. * s.fev) / c.mfev;
            {
                // :176-222 z, left to right as the reference writes it
                const double *xp = gx + (size_t) ord[s.pi] * ld, *xq = gx + (size_t) ord[s.qi] * ld,
                        *xr = gx + (size_t) ord[s.ri] * ld, *xi = gx + (size_t) ord[s.mi] * ld,
                        *xb = gx + (size_t) ord[pbest] * ld, *x0 = gx + (size_t) ord[0] * ld;
                const double *lead;
                if (c.usede) lead = s.R < 0.333 ? xp : s.R < 0.666 ? xb : x0;
                else lead = s.mi < 0.5 * s.np ? xp : xb;
                for (int i = tid; i < n; i += T) {
                    double v = lead[i] + xq[i] - xr[i] - xi[i];
                    if (c.usede) v = v + s.R * (xb[i] - xq[i]);
                    z[i] = v;
                }
                ssde_sync<T>();
                // :437-443 work = diag(b) A z
                for (int i = tid; i < n; i += T) {
                    const double b = q.ub(s.mi, i, true) < s.prank ? 1. : 0.;
                    const int o = partner[i], kind = role[i];
                    double acc = 0.;
                    if (kind == SSDE_ALONE) {
                        acc += 1. * z[i];
                    } else {
                        const double mine = SSDE_SIN * z[i];
                        const double other = (kind == SSDE_FIRST ? SSDE_COS : -SSDE_COS) * z[o];
                        if (i < o) {
                            acc += mine;
                            acc += other;
                        } else {
                            acc += other;
                            acc += mine;
                        }
                    }
                    work[i] = acc * b;
                }
                ssde_sync<T>();
                // :446-452 y = x_i + ci A' work, clamped to the box
                for (int i = tid; i < n; i += T) {
                    const int o = partner[i], kind = role[i];
                    double y = xi[i];
                    if (kind == SSDE_ALONE) {
                        y += s.ci * 1. * work[i];
                    } else {
                        // column i of A: A[i][i] = s, and A[o][i] = -c where i leads its pair, c where it follows
                        const double mine = s.ci * SSDE_SIN * work[i];
                        const double other = s.ci * (kind == SSDE_FIRST ? -SSDE_COS : SSDE_COS) * work[o];
                        if (i < o) {
                            y += mine;
                            y += other;
                        } else {
                            y += other;
                            y += mine;
                        }
                    }
                    const double ym = y < up[i] ? y : up[i];        // std::min(upper, y)
                    row[i] = lo[i] < ym ? ym : lo[i];               // std::max(lower, .)
                }
            }
            s.stage = SSDE_WAIT_SS;
            ssde_sync<T>();
            if (mode == SSDE_ADVANCE) {
                publish();
                break;
            }
        }
        if (s.stage == SSDE_WAIT_SS) {
            const double f = mode == SSDE_FUSED ? evaluate(row) : d.fcand[p];
            s.pending = 0;
            s.fev++;
            const double fi = gf[ord[s.mi]];
            bool better;
            if (select(f, better)) {
                if (better) {
                    if (tid == 0) {
                        d.SR[pm + s.lenS] = s.prank;
                        d.SC[pm + s.lenS] = s.ci;
                        d.w[pm + s.lenS] = fi - f;
                    }
                    s.lenS++;
                }
                s.mi++;
                s.stage = SSDE_MEMBER;
            } else if (c.usede) {
                s.stage = SSDE_DE;
            } else {
                s.mi++;
                s.stage = SSDE_MEMBER;
            }
            if (mode == SSDE_ABSORB) break;
        }
        if (s.stage == SSDE_DE) {
            // :253-276 the DE point: rows and draws that were known before the spherical trial's value
            if (tid == 0) {
                double zcr;
                int j0;
                q.ctrl_de(s.mi, zcr, j0);
                double cr = zcr * 0.1 + LCR[s.iL];
                cr = cr < 1. ? cr : 1.;
                cr = 0. < cr ? cr : 0.;
                bc_f[0] = cr;
                bc_i[0] = j0;
                bc_i[5] = 0;
            }
            ssde_sync<T>();
            const double CRi = bc_f[0];
            const int j0 = bc_i[0];
            const double *xp = gx + (size_t) ord[s.pi] * ld, *xq = gx + (size_t) ord[s.qi] * ld,
                    *xr = gx + (size_t) ord[s.ri] * ld, *xi = gx + (size_t) ord[s.mi] * ld, *x0 = gx + (size_t) ord[0] * ld;
            int crossed = 0;
            for (int i = tid; i < n; i += T) {
                double v;
                if (i == j0 || q.ucross(s.mi, i) <= CRi) {
                    v = xp[i] + s.R * (x0[i] - xq[i]) + s.R * (x0[i] - xr[i]);
                    if (v < lo[i] || v > up[i]) v = ssde_between(q.uredraw(s.mi, i), lo[i], up[i]);
                    crossed++;
                } else {
                    v = xi[i];
                }
                row[i] = v;
            }
            if (crossed) atomicAdd(&bc_i[5], crossed);
            ssde_sync<T>();
            // (cr1 counts in ones, :267: the sum is exact in any order)
            s.cr1 = c.repaircr ? (double) bc_i[5] / n : CRi;
            s.stage = SSDE_WAIT_DE;
            ssde_sync<T>();
            if (mode == SSDE_ADVANCE) {
                publish();
                break;
            }
        }
        if (s.stage == SSDE_WAIT_DE) {
            const double f = mode == SSDE_FUSED ? evaluate(row) : d.fcand[p];
            s.pending = 0;
            s.fev++;
            const double fi = gf[ord[s.mi]];
            bool better;
            if (select(f, better) && better) {
                if (tid == 0) {
                    d.SCR[pm + s.lenSCR] = s.cr1;
                    d.wCR[pm + s.lenSCR] = fi - f;
                }
                s.lenSCR++;
            }
            s.mi++;
            s.stage = SSDE_MEMBER;
            if (mode == SSDE_ABSORB) break;
        }
    }
    ssde_sync<T>();
    if (tid == 0) d.scal[p] = s;
}

} // namespace bbo
