// bbo_slpso_kernels.hpp -- SLPSO as gfx950 kernels.
//
//   kernel             reference lines (slpso.cpp)                                 work per population
//   slpso_init         :72-91, :211-235 the swarm, its values, abest, Uf and Pl    np rows
//   slpso_generation   :94-153 one iterate(): vdavg, alpha, the np particle steps  np + (Algorithm 2)
//                      with Algorithm 2 (:338-354), updatePar (:362-381) and       evaluations
//                      converged() (:173-189); or, entered and left at an
//                      evaluation, the part of it up to the next one
//   slpso_eval         the value of the pending point                              one row
#pragma once

#include "bbo_slpso.hpp"
#include "bbo_objectives.hpp"
#include "bbo_rng.hpp"
#include "bbo_wave.hpp"

namespace bbo {

#define SLPSO_INF (__builtin_huge_val())

enum SlpsoInitMode { SLPSO_INIT_DRAW = 1, SLPSO_INIT_EVAL = 2, SLPSO_INIT_RESET = 4, SLPSO_INIT_PAR = 8 };

// Random::get(a, b) of the reference on doubles (random.hpp:329-337) over the raw uniform u
__device__ inline double slpso_between(double u, double a, double b)
{
#pragma clang fp contract(off)
    const double lo = a < b ? a : b, hi = a < b ? b : a;
    return u * (hi - lo) + lo;
}

// The draws of one population in one generation.  The table of bbo_slpso_inject_draws and of
// "record_draws": [alpha][perm: np][np x (3 + 4 n)].  The generator's counters name what a draw is for
// -- (coordinate, particle step, generation) -- never when it is made: which branch earlier particles took
// does not move a later draw.
struct SlpsoDraws {
    const double *inj;
    double *rec;
    uint64_t seed;
    uint32_t sub, gen;
    int n, np;

    __device__ size_t step(int kp) const { return 1 + (size_t) np + (size_t) kp * (3 + 4 * (size_t) n); }
    __device__ size_t coord(int kp, int dd) const { return step(kp) + 3 + 4 * (size_t) dd; }

    __device__ double alpha() const
    {
        double a;
        if (inj) a = inj[0];
        else {
            const u32x4 w = philox4x32_10_uniform(seed, 0, 2, gen, stream_word(STREAM_SLPSO_CTRL, sub));
            a = u01(w.x, w.y);
        }
        return a;
    }
    // the forcing coin, the roulette uniform and the partner (one of the np - 1 other indices)
    __device__ void ctrl(int kp, double &uf, double &ur, int &jp) const
    {
        const size_t o = step(kp);
        if (inj) {
            uf = inj[o];
            ur = inj[o + 1];
            jp = min((int) (inj[o + 2] * (double) np), np - 1);
        } else {
            const uint32_t sw = stream_word(STREAM_SLPSO_CTRL, sub);
            const u32x4 w = philox4x32_10_uniform(seed, (uint32_t) kp, 0, gen, sw);
            const u32x4 w2 = philox4x32_10_uniform(seed, (uint32_t) kp, 1, gen, sw);
            uf = u01(w.x, w.y);
            ur = u01(w.z, w.w);
            const int r = uint_below(w2.x, np - 1);
            jp = r + (r >= kp ? 1 : 0);
        }
        if (rec) {
            rec[o] = uf;
            rec[o + 1] = ur;
            rec[o + 2] = (jp + 0.5) / np;
        }
    }
    // the uniform of the velocity (:246) and the redraw of eq. 11 (:330, :332)
    __device__ void move(int kp, int dd, double &rkd, double &ured) const
    {
        const size_t o = coord(kp, dd);
        if (inj) {
            rkd = inj[o];
            ured = inj[o + 2];
        } else {
            const u32x4 w = philox4x32_10(seed, (uint32_t) dd, (uint32_t) kp, gen, stream_word(STREAM_SLPSO_R, sub));
            rkd = u01(w.x, w.y);
            ured = u01(w.z, w.w);
        }
        if (rec) {
            rec[o] = rkd;
            rec[o + 2] = ured;
        }
    }
    // the normal of operator 1 (:261)
    __device__ double normal(int kp, int dd) const
    {
        const size_t o = coord(kp, dd);
        double z0, z1, z2, z3;
        if (inj) z0 = inj[o + 1];
        else normal_quad(seed, (uint32_t) dd | 0x20000u, (uint32_t) kp, gen, stream_word(STREAM_SLPSO_R, sub),
                    zig_global_wk(), z0, z1, z2, z3);
        if (rec) rec[o + 1] = z0;
        return z0;
    }
    // the coin of Algorithm 2 (:342)
    __device__ double coin(int kp, int dd, bool keep) const
    {
        const size_t o = coord(kp, dd);
        double u;
        if (inj) u = inj[o + 3];
        else {
            const u32x4 w = philox4x32_10(seed, (uint32_t) dd | 0x10000u, (uint32_t) kp, gen,
                    stream_word(STREAM_SLPSO_R, sub));
            u = u01(w.x, w.y);
        }
        if (rec && keep) rec[o + 3] = u;
        return u;
    }
    // Random::shuffle (:76, :365) as Fisher-Yates from one uniform per position, by ONE thread
    __device__ void shuffle(int *perm, uint32_t key) const
    {
        if (inj) {
            for (int q = 0; q < np; q++) perm[q] = (int) inj[1 + q];
        } else {
            const uint32_t sw = stream_word(STREAM_SLPSO_PERM, sub);
            for (int i = np - 1; i > 0; i--) {
                const u32x4 w = philox4x32_10_uniform(seed, (uint32_t) i, 0, key, sw);
                const int j = min((int) (u01(w.x, w.y) * (double) (i + 1)), i);
                const int t = perm[i];
                perm[i] = perm[j];
                perm[j] = t;
            }
        }
        if (rec)
            for (int q = 0; q < np; q++) rec[1 + q] = perm[q];
    }
};

// dnrm2 of the reference (blas.cpp:154-181), one thread
__device__ inline double slpso_dnrm2(int n, const double *x)
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

// converged() (:173-189) over the norms, one thread
__device__ inline int slpso_converged(const double *radius, int np, double tol)
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

// the particle's learning state as initializeParticle (:228-233) and Algorithm 3 (:404-409) leave it
__device__ inline void slpso_reset_learning(const SlpsoDev &d, size_t q)
{
    for (int i = 0; i < SLPSO_NSTRAT; i++) {
        d.p[q * 4 + i] = 0.;
        d.g[q * 4 + i] = 0;
        d.G[q * 4 + i] = 0;
        d.s[q * 4 + i] = 1. / SLPSO_NSTRAT;
    }
}

// :72-91, :211-235 for the populations p0 .. p0 + gridDim.x - 1; also what follows a set of "x" or
// "perm".  DRAW: uniform rows and the shuffled permutation; EVAL: the rows' values, a wavefront per
// row; RESET: pbest, zero velocities, the learning state, abest in index order, the counters; PAR: Uf
// and Pl from the permutation.  grid (populations), 256 threads
__global__ __launch_bounds__(256) void slpso_init(SlpsoDev d, SlpsoConst c, int p0, int mode)
{
#pragma clang fp contract(off)
    __shared__ int ibest;
    const int p = p0 + blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int n = c.n, ld = c.ld, np = c.np;
    const size_t pr = (size_t) p * np;
    double *gx = d.x + pr * ld;
    const SlpsoDraws q { nullptr, nullptr, c.seed, (uint32_t) (c.sub0 + p), 0u, n, np };
    if (mode & SLPSO_INIT_DRAW) {
        for (int r = wave; r < np; r += 4)
            for (int j = lane; j < n; j += 64) {
                const u32x4 w = philox4x32_10(c.seed, (uint32_t) r, (uint32_t) j, 0,
                        stream_word(STREAM_SLPSO_INIT, q.sub));
                gx[(size_t) r * ld + j] = slpso_between(u01(w.x, w.y), d.lower[j], d.upper[j]);
            }
        if (tid == 0) {
            int *perm = d.perm + pr;
            for (int k = 0; k < np; k++) perm[k] = k;
            q.shuffle(perm, 0u);
        }
        __syncthreads();
    }
    if (mode & SLPSO_INIT_EVAL) {
        for (int r = wave; r < np; r += 4) {
            double f = eval_row_group<64>(c.obj, n, gx + (size_t) r * ld, d.aux, lane);
            if (f != f) f = SLPSO_INF;
            if (lane == 0) d.fx[pr + r] = f;
        }
        __syncthreads();
    }
    if (mode & SLPSO_INIT_RESET) {
        for (size_t e = tid; e < (size_t) np * ld; e += 256) {
            d.pb[pr * ld + e] = gx[e];
            d.v[pr * ld + e] = 0.;
        }
        for (int k = tid; k < np; k += 256) {
            const double f = d.fx[pr + k];
            d.fpb[pr + k] = f;
            d.fp[pr + k] = f;
            d.m[pr + k] = 0;
            d.CF[pr + k] = 0;
            d.PF[pr + k] = 0;
            slpso_reset_learning(d, pr + k);
            d.radius[pr + k] = slpso_dnrm2(n, gx + (size_t) k * ld);
        }
        __syncthreads();
        if (tid == 0) {
            double fb = SLPSO_INF;
            int ib = 0;
            for (int k = 0; k < np; k++)        // :87 strict <, index order
                if (d.fx[pr + k] < fb) {
                    fb = d.fx[pr + k];
                    ib = k;
                }
            ibest = ib;
            SlpsoScal s;
            s.fabest = fb;
            s.alpha = 0.;
            s.omega = c.omegamax;
            s.mfes = 0;
            s.fev = np;
            s.it = 0;
            s.stop = 0;
            s.conv = slpso_converged(d.radius + pr, np, c.stol);
            s.stage = SLPSO_IDLE;
            s.kp = s.mv = s.iop = s.ai = s.pending = 0;
            d.scal[p] = s;
        }
        __syncthreads();
        for (int j = tid; j < ld; j += 256) {
            d.abest[(size_t) p * ld + j] = j < n ? gx[(size_t) ibest * ld + j] : 0.;
            d.vdavg[(size_t) p * ld + j] = 0.;
            d.cand[(size_t) p * ld + j] = 0.;
        }
    }
    if (mode & SLPSO_INIT_PAR) {
        for (int k = tid; k < np; k += 256) {
            const int rank = d.perm[pr + k];
            d.Uf[pr + k] = d.Uf_tab[rank];
            d.Pl[pr + k] = d.Pl_tab[rank];
        }
    }
}

// the value of the pending point.  grid (P), 64 threads
__global__ __launch_bounds__(64) void slpso_eval(SlpsoDev d, SlpsoConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    if (pop_frozen(c, d.scal + p) || !d.scal[p].pending) return;
    double f = eval_row_group<64>(c.obj, c.n, d.cand + (size_t) p * c.ld, d.aux, threadIdx.x);
    if (f != f) f = SLPSO_INF;
    if (threadIdx.x == 0) d.fcand[p] = f;
}

// the hand-over point of the workgroup's T threads
template<int T>
__device__ inline void slpso_sync()
{
    if (T == 64) wave_sync();
    else __syncthreads();
}

// updateSelectionRatios (:412-439) of particle q, one thread
__device__ inline void slpso_selection_ratios(const SlpsoDev &d, const SlpsoConst &c, size_t q, double alpha)
{
#pragma clang fp contract(off)
    double *s = d.s + q * 4, *pp = d.p + q * 4;
    int *g = d.g + q * 4, *G = d.G + q * 4;
    double sump = 0., smax = s[0], sumr = 0., r[SLPSO_NSTRAT];
    for (int i = 0; i < SLPSO_NSTRAT; i++) {
        sump += pp[i];
        if (smax < s[i]) smax = s[i];
    }
    for (int i = 0; i < SLPSO_NSTRAT; i++) {
        const double cki = (g[i] == 0 && s[i] >= smax) ? 0.9 : 1.;
        r[i] = cki * s[i];
        if (sump > 0.) r[i] += (pp[i] / sump) * alpha;
        if (G[i] > 0) r[i] += (1. * g[i]) / G[i] * (1. - alpha);
        sumr += r[i];
    }
    for (int i = 0; i < SLPSO_NSTRAT; i++) {
        s[i] = r[i] / sumr * (1. - SLPSO_NSTRAT * c.gamma) + c.gamma;
        pp[i] = 0.;
        g[i] = 0;
        G[i] = 0;
    }
}

// One iterate() of the reference per launch (mode SLPSO_FUSED), or the piece of it between two
// evaluations (SLPSO_ADVANCE, SLPSO_ABSORB): the same body, a state machine over SlpsoStage whose
// position lives in the population's scalars between launches, so the two paths run the same
// instructions on the same values.  One workgroup of T threads per population.  The lanes own the
// coordinates (velocity, position, eq. 11, the copies); thread 0 keeps the per-particle books in
// global memory and hands its decisions to the others through LDS; the first wavefront sums the
// objective from LDS with eval_row_group<64>.
// Algorithm 2 first compacts the coordinates whose coin fell below Pl into a list (the coins are keyed
// by coordinate, so the list is known before the walk).  Sequential form: coordinate after coordinate,
// abest patched in place.  Speculative form (T > 64, not SLPSO_DBG_SEQ_ALG2): the T / 64 wavefronts
// each evaluate the trial of one of the next pending coordinates against the current abest; the first
// acceptance in list order is applied, the values behind it are dropped and the walk resumes behind
// the accepted coordinate -- every value that is used is the value of the point the sequential walk
// evaluates, summed by the same routine, and fev counts the coordinates the sequential walk would
// have evaluated.
// `begin`: an idle population starts its next generation (the first SLPSO_ADVANCE of a generation).
// LDS: abest, vdavg, lower, upper, row [ld] each, (T > 64) T / 64 trial rows [ld], the list [ld] ints.
// grid (P), T threads
template<int T>
__global__ __launch_bounds__(T) void slpso_generation(SlpsoDev d, SlpsoConst c, int mode, int begin)
{
#pragma clang fp contract(off)
    constexpr int W = T / 64;
    extern __shared__ double slpso_lds[];
    __shared__ double bc_f[W + 2];
    __shared__ int bc_i[4];
    __shared__ int chunk_cnt[SLPSO_MAX_N / 64];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = c.n, ld = c.ld, np = c.np;
    SlpsoScal s = d.scal[p];
    if (pop_frozen(c, &s)) return;
    if (mode == SLPSO_ABSORB && !s.pending) return;
    if (mode == SLPSO_ADVANCE && s.pending) return;     // (a value is still owed)
    // (a population that has completed its generation waits for the others of the handle)
    if (mode == SLPSO_ADVANCE && s.stage == SLPSO_IDLE && !begin) return;
    const size_t pr = (size_t) p * np;
    double *gx = d.x + pr * ld, *gv = d.v + pr * ld, *gpb = d.pb + pr * ld;
    double *abest = slpso_lds, *vdavg = abest + ld, *lo = vdavg + ld, *up = lo + ld, *row = up + ld;
    double *trial = row + ld;
    int *plist = reinterpret_cast<int*>(trial + (W > 1 ? W * ld : 0));
    const size_t tlen = 1 + (size_t) np + (size_t) np * (3 + 4 * (size_t) n);
    SlpsoDraws q { d.inject ? d.inject + (size_t) p * tlen : nullptr, d.draws ? d.draws + (size_t) p * tlen : nullptr,
            c.seed, (uint32_t) (c.sub0 + p), (uint32_t) s.it, n, np };
    const bool speculative = W > 1 && !(c.dbg & SLPSO_DBG_SEQ_ALG2);

    if (mode == SLPSO_FUSED && s.stage == SLPSO_WAIT_ALG2) s.stage = SLPSO_ALG2;    // (the walk evaluates it itself)
    if (mode == SLPSO_FUSED) s.pending = 0;
    for (int i = tid; i < n; i += T) {
        lo[i] = d.lower[i];
        up[i] = d.upper[i];
        abest[i] = d.abest[(size_t) p * ld + i];
        vdavg[i] = d.vdavg[(size_t) p * ld + i];
        if (s.stage == SLPSO_WAIT_MOVE) row[i] = gx[(size_t) s.mv * ld + i];
    }
    slpso_sync<T>();

    // the value of a row in LDS, in every thread
    auto evaluate = [&](const double *r) {
        double f = 0.;
        if (wave == 0) {
            f = eval_row_group<64>(c.obj, n, r, d.aux, lane);
            if (f != f) f = SLPSO_INF;
            if (W > 1 && lane == 0) bc_f[W] = f;
        }
        if (W > 1) {
            __syncthreads();
            f = bc_f[W];
            __syncthreads();
        }
        return f;
    };
    // :134-149 for the moved particle: pbest, abest, the selection ratios
    auto finish_particle = [&]() {
        const size_t k = pr + s.mv;
        if (tid == 0) {
            const double f = d.fx[k];
            const int upb = f < d.fpb[k] ? 1 : 0;
            if (upb) d.fpb[k] = f;
            bc_i[0] = upb;
            bc_i[1] = upb && f < s.fabest ? 1 : 0;
            bc_f[W + 1] = f;
            if (d.m[k] >= d.Uf[k]) slpso_selection_ratios(d, c, k, s.alpha);
        }
        slpso_sync<T>();
        const int upb = bc_i[0], uab = bc_i[1];
        const double f = bc_f[W + 1];
        if (upb)
            for (int i = tid; i < n; i += T) {
                const double v = gx[(size_t) s.mv * ld + i];
                gpb[(size_t) s.mv * ld + i] = v;
                if (uab) abest[i] = v;
            }
        if (uab) s.fabest = f;
        slpso_sync<T>();
        s.kp++;
        s.stage = SLPSO_MOVE;
    };
    // the coordinates of Algorithm 2 whose coin fell below Pl, in order: plist[0 .. npend)
    int npend = 0;
    bool listed = false;
    auto build_list = [&]() {
        const double Pl = d.Pl[pr + s.mv];
        const int nchunks = (n + 63) / 64;
        for (int ch = wave; ch < nchunks; ch += W) {
            const int dd = ch * 64 + lane;
            const bool flag = dd < n && q.coin(s.kp, dd, true) < Pl;
            const unsigned long long mask = __ballot(flag);
            if (lane == 0) chunk_cnt[ch] = __popcll(mask);
        }
        slpso_sync<T>();
        npend = 0;
        for (int ch = 0; ch < nchunks; ch++) npend += chunk_cnt[ch];
        for (int ch = wave; ch < nchunks; ch += W) {
            const int dd = ch * 64 + lane;
            const bool flag = dd < n && q.coin(s.kp, dd, false) < Pl;
            const unsigned long long mask = __ballot(flag);
            int off = 0;
            for (int e = 0; e < ch; e++) off += chunk_cnt[e];
            if (flag) plist[off + __popcll(mask & ((1ull << lane) - 1ull))] = dd;
        }
        slpso_sync<T>();
        listed = true;
    };

    for (;;) {
        if (s.stage == SLPSO_IDLE) {
            if (mode == SLPSO_ABSORB) break;
            // :97-105 vdavg in swarm order, alpha
            if (q.rec) {
                for (size_t e = tid; e < tlen; e += T) q.rec[e] = 0.;
                slpso_sync<T>();
            }
            for (int i = tid; i < n; i += T) {
                double acc = 0.;
                for (int k = 0; k < np; k++) acc += fabs(gv[(size_t) k * ld + i]) / np;
                vdavg[i] = acc;
            }
            s.alpha = q.alpha();
            if (q.rec && tid == 0) q.rec[0] = s.alpha;
            s.kp = 0;
            s.stage = SLPSO_MOVE;
            slpso_sync<T>();
        }
        if (s.stage == SLPSO_MOVE) {
            if (s.kp >= np) {
                // updatePar (:362-381), converged() (:173-189), the budget (:163)
                if (tid == 0) q.shuffle(d.perm + pr, (uint32_t) s.it + 1u);
                slpso_sync<T>();
                const double r0 = (1. * s.fev) / c.mfev;
                const double r1 = 1. < r0 ? 1. : r0;
                const double pfev = 0. < r1 ? r1 : 0.;
                s.mfes = (int) (np * (1. - exp(-100. * pow(pfev, 3.))));
                for (int k = tid; k < np; k += T) {
                    const size_t e = pr + k;
                    const int rank = d.perm[e];
                    d.Uf[e] = d.Uf_tab[rank];
                    d.Pl[e] = d.Pl_tab[rank];
                    const int CF = d.CF[e], PF = d.PF[e];
                    if (!CF && PF) {                // Algorithm 3
                        double *sv = d.s + e * 4;
                        const double sum = ((0. + sv[0]) + sv[1]) + sv[2];
                        sv[0] /= sum;
                        sv[1] /= sum;
                        sv[2] /= sum;
                        sv[3] = 0.;
                    }
                    if (CF && !PF) slpso_reset_learning(d, e);
                    d.radius[e] = slpso_dnrm2(n, gx + (size_t) k * ld);
                }
                s.omega = c.omegamax - (c.omegamax - c.omegamin) * pfev;
                s.it++;
                slpso_sync<T>();
                if (tid == 0) bc_i[0] = slpso_converged(d.radius + pr, np, c.stol);
                slpso_sync<T>();
                s.conv = bc_i[0];
                if (s.conv) s.stop = 1;
                else if (s.fev >= c.mfev) s.stop = 2;
                s.stage = SLPSO_IDLE;
                s.pending = 0;
                break;
            }
            // :110-117 the operator; Algorithm 1 (:237-323) picks who moves and towards what
            if (tid == 0) {
                const size_t k = pr + s.kp;
                d.PF[k] = d.CF[k];
                double uf, ur;
                int jp, iop = SLPSO_NSTRAT - 1;
                q.ctrl(s.kp, uf, ur, jp);
                if (!(np * uf < s.mfes)) {
                    const double *sv = d.s + k * 4;
                    const double sum = (((0. + sv[0]) + sv[1]) + sv[2]) + sv[3];
                    double U = slpso_between(ur, 0., sum);
                    for (int i = 0; i < SLPSO_NSTRAT; i++) {
                        U -= sv[i];
                        if (U <= 0.) {
                            iop = i;
                            break;
                        }
                    }
                }
                d.CF[k] = iop == SLPSO_NSTRAT - 1 ? 1 : 0;
                int mv = s.kp, tgt = s.kp;          // tgt: the row of pbest to learn from (-1: abest)
                if (iop == 3) tgt = -1;
                if (iop == 2) {
                    if (d.fpb[pr + jp] < d.fpb[k]) tgt = jp;
                    else mv = jp;
                }
                d.fp[pr + mv] = d.fx[pr + mv];
                bc_i[0] = iop;
                bc_i[1] = mv;
                bc_i[2] = tgt;
            }
            slpso_sync<T>();
            s.iop = bc_i[0];
            s.mv = bc_i[1];
            const int tgt = bc_i[2];
            for (int i = tid; i < n; i += T) {
                const size_t e = (size_t) s.mv * ld + i;
                const double x = gx[e];
                double rkd, ured, step;
                q.move(s.kp, i, rkd, ured);
                if (s.iop == 1) {
                    step = vdavg[i] * q.normal(s.kp, i);
                } else {
                    const double t = tgt < 0 ? abest[i] : gpb[(size_t) tgt * ld + i];
                    double vn = s.omega * gv[e] + c.eta * rkd * (t - x);
                    const double vmax = c.vmax * (up[i] - lo[i]);
                    vn = vmax < vn ? vmax : vn;
                    vn = -vmax < vn ? vn : -vmax;
                    gv[e] = vn;
                    step = vn;
                }
                const double x1 = x + step;       // eq. 11 (:325-336)
                double xn = x1;
                if (x1 < lo[i]) xn = slpso_between(ured, lo[i], x);
                else if (x1 > up[i]) xn = slpso_between(ured, x, up[i]);
                gx[e] = xn;
                row[i] = xn;
            }
            s.stage = SLPSO_WAIT_MOVE;
            slpso_sync<T>();
            if (mode == SLPSO_ADVANCE) {
                for (int i = tid; i < n; i += T) d.cand[(size_t) p * ld + i] = row[i];
                s.pending = 1;
                break;
            }
        }
        if (s.stage == SLPSO_WAIT_MOVE) {
            const double f = mode == SLPSO_FUSED ? evaluate(row) : d.fcand[p];
            s.pending = 0;
            s.fev++;
            if (tid == 0) {                     // :123-131
                const size_t k = pr + s.mv;
                d.fx[k] = f;
                d.G[k * 4 + s.iop]++;
                const double fp = d.fp[k];
                const int better = f < fp ? 1 : 0;
                if (better) {
                    d.g[k * 4 + s.iop]++;
                    d.m[k] = 0;
                    d.p[k * 4 + s.iop] += (fp - f);
                } else {
                    d.m[k]++;
                }
                bc_i[3] = better;
            }
            slpso_sync<T>();
            const int better = bc_i[3];
            if (better) {
                s.stage = SLPSO_ALG2;
                s.ai = 0;
                listed = false;
            } else {
                finish_particle();
            }
            if (mode == SLPSO_ABSORB) break;
        }
        if (s.stage == SLPSO_ALG2) {
            if (!listed) build_list();
            if (mode == SLPSO_FUSED && speculative && s.ai < npend) {
                for (int e = tid; e < W * n; e += T) trial[(e / n) * ld + (e % n)] = abest[e % n];
                __syncthreads();
                while (s.ai < npend) {
                    const int cnt = min(W, npend - s.ai);
                    int dd = 0;
                    if (wave < cnt) {
                        dd = plist[s.ai + wave];
                        if (lane == 0) trial[wave * ld + dd] = gx[(size_t) s.mv * ld + dd];
                        wave_sync();
                        double fw = eval_row_group<64>(c.obj, n, trial + wave * ld, d.aux, lane);
                        if (fw != fw) fw = SLPSO_INF;
                        if (lane == 0) bc_f[wave] = fw;
                    }
                    __syncthreads();
                    int acc = -1;
                    for (int w = 0; w < cnt; w++)
                        if (bc_f[w] < s.fabest) {
                            acc = w;
                            break;
                        }
                    const double facc = acc >= 0 ? bc_f[acc] : 0.;
                    if (wave < cnt && lane == 0) trial[wave * ld + dd] = abest[dd];
                    __syncthreads();
                    if (acc >= 0) {
                        const int da = plist[s.ai + acc];
                        const double xa = gx[(size_t) s.mv * ld + da];
                        s.fabest = facc;
                        if (tid < W) trial[tid * ld + da] = xa;
                        if (tid == W) abest[da] = xa;
                    }
                    const int used = acc >= 0 ? acc + 1 : cnt;
                    s.ai += used;
                    s.fev += used;
                    __syncthreads();
                }
            } else if (mode == SLPSO_FUSED) {
                while (s.ai < npend) {          // :341-353, one chosen coordinate after another
                    const int dd = plist[s.ai];
                    double old = 0.;
                    if (tid == 0) {
                        old = abest[dd];
                        abest[dd] = gx[(size_t) s.mv * ld + dd];
                    }
                    slpso_sync<T>();
                    const double f = evaluate(abest);
                    s.fev++;
                    s.ai++;
                    if (f < s.fabest) s.fabest = f;
                    else if (tid == 0) abest[dd] = old;
                    slpso_sync<T>();
                }
            }
            if (s.ai >= npend) {
                finish_particle();
                continue;
            }
            // (SLPSO_ADVANCE) the trial of the next chosen coordinate
            const int dd = plist[s.ai];
            for (int i = tid; i < n; i += T)
                d.cand[(size_t) p * ld + i] = i == dd ? gx[(size_t) s.mv * ld + dd] : abest[i];
            s.stage = SLPSO_WAIT_ALG2;
            s.pending = 1;
            break;
        }
        if (s.stage == SLPSO_WAIT_ALG2) {       // (SLPSO_ABSORB) :346-351
            if (!listed) build_list();
            const double f = d.fcand[p];
            const int dd = plist[s.ai];
            if (f < s.fabest) {
                s.fabest = f;
                if (tid == 0) abest[dd] = gx[(size_t) s.mv * ld + dd];
            }
            s.fev++;
            s.ai++;
            s.stage = SLPSO_ALG2;
            s.pending = 0;
            slpso_sync<T>();
            break;
        }
    }
    slpso_sync<T>();
    for (int i = tid; i < n; i += T) {
        d.abest[(size_t) p * ld + i] = abest[i];
        d.vdavg[(size_t) p * ld + i] = vdavg[i];
    }
    if (tid == 0) d.scal[p] = s;
}

} // namespace bbo
