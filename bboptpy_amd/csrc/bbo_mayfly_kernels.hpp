// bbo_mayfly_kernels.hpp -- the mayfly optimizer as gfx950 kernels.
//
//   kernel            reference lines (mayfly.cpp)                                work per population
//   mayfly_init       :81-131 uniform males and females and their values          2 np rows
//   mayfly_init_best  :97-122 fbest and best in the order male j, female j        2 np values
//   mayfly_begin      :224, :238 the two shuffles as permutations                 np + nmut indices
//   mayfly_females    :168-172, :331-367 female move and value                    np rows, a wavefront each
//   mayfly_males      :174-199, :303-329 the females' fbest chain (pgb), then the
//                     male loop as prefix-commit rounds                           np rows + the redone ones
//   mayfly_rank       :202-203, :249, :268 stable order of a swarm / a selection  np or cm values
//   mayfly_cross      :206-211, :375-398 two offspring per pair and their values  np rows
//   mayfly_mutate     :226-230, :400-428 mutated flies and their values           nmut rows
//   mayfly_merge      :213-219, :232-236 fbest chain of offspring and mutated
//                     flies; the values the two selections sort                   2 cm values
//   mayfly_resolve    :250-258, :269-275 the record that lands in every slot of
//                     the in-place copy loop; :277-281 the schedule, the budget   2 np integers
//   mayfly_copy       the rows of the selected records into the other buffer      2 np rows
#pragma once

#include "bbo_mayfly.hpp"
#include "bbo_objectives.hpp"
#include "bbo_rank.hpp"
#include "bbo_rng.hpp"
#include "bbo_wave.hpp"

namespace bbo {

#define MAYFLY_INF (__builtin_huge_val())

enum MayflyInitMode { MAYFLY_INIT_DRAW = 1, MAYFLY_INIT_EVAL = 2 };

constexpr int MAYFLY_INIT_ROWS = 64;    // rows per workgroup of mayfly_init
constexpr int MAYFLY_RANK_CANDS = 32;   // candidates per workgroup of mayfly_rank (rank_by_counting<8>)

// The draw table of one generation and population (bbo_mayfly_inject_draws, "draws"), in doubles:
//   uf [np][n]   canonical uniforms of the females' random flights (-1: the female took the other form)
//   um [np][n]   the same of the males' nuptial dances
//   po [np]      the shuffle of the offspring: shuffled place -> offspring
//   pu [nmut]    the shuffle of the mutated flies
//   ix [nmut][nmd], z [nmut][nmd]   per mutated fly the displaced genes and their normals
struct MayflyTable {
    size_t uf, um, po, pu, ix, z, len;
};

__host__ __device__ inline MayflyTable mayfly_table(int n, int np, int nmut, int nmd)
{
    MayflyTable t;
    t.uf = 0;
    t.um = (size_t) np * n;
    t.po = 2 * (size_t) np * n;
    t.pu = t.po + np;
    t.ix = t.pu + nmut;
    t.z = t.ix + (size_t) nmut * nmd;
    t.len = t.z + (size_t) nmut * nmd;
    return t;
}

// std::min / std::max as the reference calls them
__device__ inline double mayfly_clamp(double v, double lo, double hi)
{
    const double m = hi < v ? hi : v;
    return m < lo ? lo : m;
}

// Keyed bijection of [0, range): the Feistel network of cso_perm with a tag in the counter, so that the
// shuffles of one generation (tag 0 offspring, 1 mutated flies, 2 + u the genes of mutated fly u) differ
__device__ inline uint32_t mayfly_perm(uint32_t s0, int kb, uint32_t range, uint64_t seed, uint32_t tag,
        uint32_t gen, uint32_t sw)
{
    const uint32_t mask = (1u << kb) - 1u;
    uint32_t x = s0;
    do {
        uint32_t L = x >> kb, R = x & mask;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const u32x4 w = philox4x32_10(seed, R, (uint32_t) (8 + r) | (tag << 8), gen, sw);
            const uint32_t t = L ^ (w.x & mask);
            L = R;
            R = t;
        }
        x = (L << kb) | R;
    } while (x >= range);
    return x;
}

// Random::get(-1., 1.) of coordinate i of fly j (blk 0: the females, 1: the males): addressed by what it
// is for, so a male that is formed again draws the same
__device__ inline double mayfly_flight(const MayflyDev &d, const MayflyConst &c, int p, int blk, int j, int i,
        uint32_t gen)
{
#pragma clang fp contract(off)
    const size_t at = (size_t) p * c.table + (blk ? (size_t) c.np * c.n : 0) + (size_t) j * c.n + i;
    double u;
    if (d.inject) {
        u = d.inject[at];
    } else {
        const u32x4 w = philox4x32_10(c.seed, (uint32_t) i, (uint32_t) j | ((uint32_t) blk << 16), gen,
                stream_word(STREAM_MAYFLY_R, (uint32_t) (c.sub0 + p)));
        u = u01(w.x, w.y);
    }
    if (d.draws) d.draws[at] = u;
    return u * 2. + -1.;
}

__device__ inline void mayfly_no_flight(const MayflyDev &d, const MayflyConst &c, int p, int blk, int j, int i)
{
    if (d.draws) d.draws[(size_t) p * c.table + (blk ? (size_t) c.np * c.n : 0) + (size_t) j * c.n + i] = -1.;
}

// the value of a row in global memory that this wavefront has just written
__device__ inline double mayfly_value(const MayflyDev &d, const MayflyConst &c, const double *x, int lane)
{
#pragma clang fp contract(off)
    wave_sync();
    double f = eval_row_group<64>(c.obj, c.n, x, d.aux, lane);
    if (f != f) f = MAYFLY_INF;
    return f;
}

// :81-131 for the populations p0 .. p0 + gridDim.x - 1, a wavefront per row; blockIdx.z: 0 males, 1 females.
// The reference builds its flies as mayfly { v, x, bx, f, f } over a struct declared _x, _v, _bx (:93, :112):
// the drawn point becomes the VELOCITY and the zero vector the position, so every fly starts at the origin
// with the value of the point it drew (a male's own best is that point).  repair: x = the point, v = 0.
// grid (populations, ceil(np / MAYFLY_INIT_ROWS), 2), 256 threads
__device__ inline double *mayfly_drawn(const MayflyDev &d, const MayflyConst &c, int fem, size_t row)
{
    return (c.repair ? (fem ? d.FX : d.MX) : (fem ? d.FV : d.MV)) + row;
}

__global__ __launch_bounds__(256) void mayfly_init(MayflyDev d, MayflyConst c, int p0, int mode)
{
#pragma clang fp contract(off)
    const int p = p0 + blockIdx.x, fem = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = c.n, np = c.np;
    const int r1 = min(np, ((int) blockIdx.y + 1) * MAYFLY_INIT_ROWS);
    for (int r = blockIdx.y * MAYFLY_INIT_ROWS + wave; r < r1; r += 4) {
        const size_t row = ((size_t) p * np + r) * c.ld;
        double *x = mayfly_drawn(d, c, fem, row);
        double *zero = (c.repair ? (fem ? d.FV : d.MV) : (fem ? d.FX : d.MX)) + row;
        if (mode & MAYFLY_INIT_DRAW) {
            for (int j = lane; j < c.ld; j += 64) {
                double v = 0.;
                if (j < n) {
                    const u32x4 w = philox4x32_10(c.seed, (uint32_t) r | ((uint32_t) fem << 16), (uint32_t) j, 0,
                            stream_word(STREAM_MAYFLY_INIT, (uint32_t) (c.sub0 + p)));
                    const double a = d.lower[j], b = d.upper[j];
                    const double lo = a < b ? a : b, hi = a < b ? b : a;
                    v = u01(w.x, w.y) * (hi - lo) + lo;
                }
                x[j] = v;
                zero[j] = 0.;
                if (!fem) d.MBX[row + j] = v;
            }
        }
        if (mode & MAYFLY_INIT_EVAL) {
            const double f = mayfly_value(d, c, x, lane);
            if (lane == 0) {
                if (fem) d.Ff[(size_t) p * np + r] = f;
                else d.Mf[(size_t) p * np + r] = f;
            }
        }
    }
}

// :97-122: fbest and best over male 0, female 0, male 1, ... (the females under pgb only), the first of
// equal values; the males' own best values.  grid (populations), 64 threads
__global__ __launch_bounds__(64) void mayfly_init_best(MayflyDev d, MayflyConst c, int p0)
{
    const int p = p0 + blockIdx.x, lane = threadIdx.x, np = c.np;
    double v = MAYFLY_INF;
    int at = 0x7fffffff;
    for (int q = lane; q < 2 * np; q += 64) {
        const int j = q >> 1;
        double f = MAYFLY_INF;
        if (!(q & 1)) {
            f = d.Mf[(size_t) p * np + j];
            d.Mbf[(size_t) p * np + j] = f;
        } else if (c.pgb) {
            f = d.Ff[(size_t) p * np + j];
        }
        if (f < v) {
            v = f;
            at = q;
        }
    }
    wave_argmin(v, at);
    if (at == 0x7fffffff) at = 0;       // (every value +inf: the reference keeps its zero vector; here male 0)
    const double *x = mayfly_drawn(d, c, at & 1, ((size_t) p * np + (at >> 1)) * c.ld);
    for (int i = lane; i < c.ld; i += 64) d.best[(size_t) p * c.ld + i] = i < c.n ? x[i] : 0.;
    if (lane == 0) d.scal[p].fbest = v;
}

// The head of a generation: whether it runs in this population, and the two shuffles (:224, :238) as
// permutations.  grid (P), 256 threads
__global__ __launch_bounds__(256) void mayfly_begin(MayflyDev d, MayflyConst c)
{
    const int p = blockIdx.x, tid = threadIdx.x;
    MayflyScal *sc = d.scal + p;
    const bool on = !pop_frozen(c, sc);
    __syncthreads();
    if (tid == 0) {
        sc->active = on ? 1 : 0;
        if (on) sc->took = -1;
    }
    if (!on) return;
    const MayflyTable t = mayfly_table(c.n, c.np, c.nmut, c.nmd);
    const uint32_t gen = (uint32_t) sc->it, sw = stream_word(STREAM_MAYFLY_PERM, (uint32_t) (c.sub0 + p));
    const size_t tb = (size_t) p * c.table;
    for (int q = tid; q < c.np + c.nmut; q += 256) {
        const bool off = q < c.np;
        const int k = off ? q : q - c.np, range = off ? c.np : c.nmut;
        const size_t at = tb + (off ? t.po : t.pu) + k;
        int v;
        if (d.inject) v = min(max((int) d.inject[at], 0), range - 1);
        else v = (int) mayfly_perm((uint32_t) k, off ? c.kb_np : c.kb_nmut, (uint32_t) range, c.seed, off ? 0u : 1u, gen, sw);
        (off ? d.permo : d.permu)[(size_t) p * range + k] = v;
        if (d.draws) d.draws[at] = (double) v;
    }
}

// :168-172, :331-367: female j against male j.  r is summed in the reference's order by every lane.
// grid (np, P), 64 threads
__global__ __launch_bounds__(64) void mayfly_females(MayflyDev d, MayflyConst c)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
    const MayflyScal *sc = d.scal + p;
    if (!sc->active) return;
    const int n = c.n, np = c.np;
    const size_t row = ((size_t) p * np + j) * c.ld;
    double *xf = d.FX + row, *vf = d.FV + row;
    const double *xm = d.MX + row;
    double r = 0.;
    for (int i = 0; i < n; i++) {
        const double dd = xf[i] - xm[i];
        r += dd * dd;
    }
    const bool attract = d.Mf[(size_t) p * np + j] < d.Ff[(size_t) p * np + j];
    const double g = sc->g, fl = sc->fl;
    const double e = c.a3 * exp(-c.beta * r);
    const uint32_t gen = (uint32_t) sc->it;
    for (int i = lane; i < n; i += 64) {
        double v = vf[i];
        const double x = xf[i];
        if (attract) {
            v = g * v + e * (xm[i] - x);
            mayfly_no_flight(d, c, p, 0, j, i);
        } else {
            v = g * v + fl * mayfly_flight(d, c, p, 0, j, i, gen);
        }
        const double vmax = c.vdamp * (d.upper[i] - d.lower[i]);
        v = mayfly_clamp(v, -vmax, vmax);
        vf[i] = v;
        xf[i] = mayfly_clamp(x + v, d.lower[i], d.upper[i]);
    }
    if (lane == 0) d.brf[(size_t) p * np + j] = attract ? 1 : 0;
    if (c.obj != OBJ_HOST) {
        const double f = mayfly_value(d, c, xf, lane);
        if (lane == 0) d.Ff[(size_t) p * np + j] = f;
    }
}

// :303-329 and the move of :356-362 for male j by one wavefront, into the candidate rows cx, cv: nothing
// of the male itself is written, so a male formed ahead of its turn can be dropped
__device__ inline void mayfly_form_male(const MayflyDev &d, const MayflyConst &c, const MayflyScal *sc, int p, int j,
        int lane, double fbest, double *cx, double *cv)
{
#pragma clang fp contract(off)
    const int n = c.n, np = c.np;
    const size_t row = ((size_t) p * np + j) * c.ld;
    const double *x = d.MX + row, *v0 = d.MV + row, *bx = d.MBX + row, *best = d.best + (size_t) p * c.ld;
    double rp = 0., rg = 0.;
    for (int i = 0; i < n; i++) {
        const double dp = bx[i] - x[i], dg = best[i] - x[i];
        rp += dp * dp;
        rg += dg * dg;
    }
    const bool attract = d.Mf[(size_t) p * np + j] > fbest;
    const double g = sc->g, dance = sc->dance;
    const double e1 = c.a1 * exp(-c.beta * rp), e2 = c.a2 * exp(-c.beta * rg);
    const uint32_t gen = (uint32_t) sc->it;
    for (int i = lane; i < n; i += 64) {
        double v = v0[i];
        const double xi = x[i];
        if (attract) {
            v = g * v + e1 * (bx[i] - xi) + e2 * (best[i] - xi);
            mayfly_no_flight(d, c, p, 1, j, i);
        } else {
            v = g * v + dance * mayfly_flight(d, c, p, 1, j, i, gen);
        }
        const double vmax = c.vdamp * (d.upper[i] - d.lower[i]);
        v = mayfly_clamp(v, -vmax, vmax);
        cv[i] = v;
        cx[i] = mayfly_clamp(xi + v, d.lower[i], d.upper[i]);
    }
    if (lane == 0) d.brm[(size_t) p * np + j] = attract ? 1 : 0;
}

// The females' fbest chain under pgb (:174-179), then the male loop (:183-199) as prefix-commit rounds:
// the next `window` males are formed and evaluated against the current best, a wavefront each; they are
// committed up to and including the first whose own best beats fbest, which becomes the new best, and the
// rest is formed again.  The result is the sequential loop's: a male is committed only when every male
// before it is, and no committed male before it changed best or fbest after it was formed.
//   mode   MAYFLY_FUSED: the whole loop.  MAYFLY_FORM: male `jm` into candidate slot 0 (before male 0 the
//          females' chain).  MAYFLY_ABSORB: commit male `jm` with the value the host put into candf.
// grid (P), MAYFLY_WG threads
__global__ __launch_bounds__(MAYFLY_WG) void mayfly_males(MayflyDev d, MayflyConst c, int mode)
{
#pragma clang fp contract(off)
    __shared__ double sval[4];
    __shared__ int sidx[4];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    MayflyScal *sc = d.scal + p;
    if (!sc->active) return;
    const int n = c.n, np = c.np, ld = c.ld;
    double fbest = sc->fbest;
    int took = -1, dropped = 0, rounds = 0;
    int j0 = mode == MAYFLY_FUSED ? 0 : sc->jm;
    const int jend = mode == MAYFLY_FUSED ? np : j0 + 1;
    const int W = mode == MAYFLY_FUSED ? c.window : 1;
    double *best = d.best + (size_t) p * ld;
    double *Mf = d.Mf + (size_t) p * np, *Mbf = d.Mbf + (size_t) p * np;
    double *candx = d.candx + (size_t) p * c.window * ld, *candv = d.candv + (size_t) p * c.window * ld;
    double *candf = d.candf + (size_t) p * c.window;
    __syncthreads();

    if (c.pgb && mode != MAYFLY_ABSORB && j0 == 0) {
        double v = MAYFLY_INF;
        int at = 0x7fffffff;
        for (int j = tid; j < np; j += MAYFLY_WG) {
            const double f = d.Ff[(size_t) p * np + j];
            if (f < v) {
                v = f;
                at = j;
            }
        }
        block_arg<1>(v, at, sval, sidx);
        if (v < fbest) {
            fbest = v;
            took = at;
            const double *x = d.FX + ((size_t) p * np + at) * ld;
            for (int i = tid; i < n; i += MAYFLY_WG) best[i] = x[i];
        }
        __syncthreads();
    }

    while (j0 < jend) {
        const int cnt = min(W, jend - j0);
        if (mode != MAYFLY_ABSORB) {
            for (int w = wave; w < cnt; w += MAYFLY_WG / 64) {
                mayfly_form_male(d, c, sc, p, j0 + w, lane, fbest, candx + (size_t) w * ld, candv + (size_t) w * ld);
                if (mode == MAYFLY_FUSED) {
                    const double f = mayfly_value(d, c, candx + (size_t) w * ld, lane);
                    if (lane == 0) candf[w] = f;
                }
            }
        }
        if (mode == MAYFLY_FORM) break;
        __syncthreads();
        // the males of the round that stand: up to the first whose own best beats fbest
        int commit = cnt, improver = -1;
        for (int w = 0; w < cnt; w++) {
            const double f = candf[w], bf = Mbf[j0 + w];
            if ((f < bf ? f : bf) < fbest) {
                commit = w + 1;
                improver = w;
                break;
            }
        }
        __syncthreads();
        for (int w = wave; w < commit; w += MAYFLY_WG / 64) {
            const size_t row = ((size_t) p * np + j0 + w) * ld;
            const double f = candf[w];
            const bool better = f < Mbf[j0 + w];
            for (int i = lane; i < n; i += 64) {
                const double xi = candx[(size_t) w * ld + i];
                d.MX[row + i] = xi;
                d.MV[row + i] = candv[(size_t) w * ld + i];
                if (better) d.MBX[row + i] = xi;
            }
            wave_sync();
            if (lane == 0) {
                Mf[j0 + w] = f;
                if (better) Mbf[j0 + w] = f;
            }
        }
        __syncthreads();
        if (improver >= 0) {
            const int jj = j0 + improver;
            fbest = Mbf[jj];
            took = np + jj;
            const double *bx = d.MBX + ((size_t) p * np + jj) * ld;
            for (int i = tid; i < n; i += MAYFLY_WG) best[i] = bx[i];
        }
        __syncthreads();
        dropped += cnt - commit;
        rounds++;
        j0 += commit;
    }

    if (tid == 0) {
        sc->fbest = fbest;
        if (took >= 0) sc->took = took;
        sc->dropped += dropped;
        sc->rounds += rounds;
        if (mode == MAYFLY_ABSORB) sc->jm = j0 >= np ? 0 : j0;
    }
}

// The stable order (bbo_rank.hpp) of a swarm by value (which 0: blockIdx.z 0 the males, 1 the females) or of
// the records of a selection (which 1).  grid (P, ceil(count / MAYFLY_RANK_CANDS), 2), 256 threads
__global__ __launch_bounds__(256) void mayfly_rank(MayflyDev d, MayflyConst c, int which)
{
    __shared__ double tile[RANK_TILE];
    const int p = blockIdx.x, fem = blockIdx.z;
    if (!d.scal[p].active) return;
    const int count = which ? c.cm : c.np;
    const double *f = which ? d.keys + ((size_t) p * 2 + fem) * c.cm : (fem ? d.Ff : d.Mf) + (size_t) p * c.np;
    int *out = which ? d.ordt + ((size_t) p * 2 + fem) * c.cm : (fem ? d.ordf : d.ordm) + (size_t) p * c.np;
    const int cand = blockIdx.y * MAYFLY_RANK_CANDS + (threadIdx.x >> 3), slice = threadIdx.x & 7;
    const int r = rank_by_counting<8>(f, count, cand, slice, tile);
    if (cand < count && slice == 0 && r < count) out[r] = cand;
}

// :206-211, :375-398: offspring k of pair k / 2 (even k: l male + (1 - l) female, odd k the other way round).
// grid (np, P), 64 threads
__global__ __launch_bounds__(64) void mayfly_cross(MayflyDev d, MayflyConst c)
{
#pragma clang fp contract(off)
    const int k = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
    if (!d.scal[p].active) return;
    const int n = c.n, np = c.np;
    const int pm = min(max(d.ordm[(size_t) p * np + (k >> 1)], 0), np - 1);
    const int pf = min(max(d.ordf[(size_t) p * np + (k >> 1)], 0), np - 1);
    const double *xm = d.MX + ((size_t) p * np + pm) * c.ld, *xf = d.FX + ((size_t) p * np + pf) * c.ld;
    const double *a = (k & 1) ? xf : xm, *b = (k & 1) ? xm : xf;
    double *o = d.OX + ((size_t) p * np + k) * c.ld;
    for (int i = lane; i < n; i += 64)
        o[i] = mayfly_clamp(c.l * a[i] + (1. - c.l) * b[i], d.lower[i], d.upper[i]);
    if (c.obj != OBJ_HOST) {
        const double f = mayfly_value(d, c, o, lane);
        if (lane == 0) d.Of[(size_t) p * np + k] = f;
    }
}

// :226-230, :400-428: mutated fly u from the offspring at shuffled place u; nmd genes displaced.
// grid (nmut, P), 64 threads
__global__ __launch_bounds__(64) void mayfly_mutate(MayflyDev d, MayflyConst c)
{
#pragma clang fp contract(off)
    const int u = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
    const MayflyScal *sc = d.scal + p;
    if (!sc->active) return;
    const int n = c.n, np = c.np, nmd = c.nmd;
    const MayflyTable t = mayfly_table(n, np, c.nmut, nmd);
    const int par = min(max(d.permo[(size_t) p * np + u], 0), np - 1);
    const double *px = d.OX + ((size_t) p * np + par) * c.ld;
    double *o = d.UX + ((size_t) p * c.nmut + u) * c.ld;
    for (int i = lane; i < n; i += 64) o[i] = px[i];
    wave_sync();
    const uint32_t gen = (uint32_t) sc->it;
    const size_t tb = (size_t) p * c.table;
    for (int q = lane; q < nmd; q += 64) {
        const size_t at = (size_t) u * nmd + q;
        int k;
        double z;
        if (d.inject) {
            k = min(max((int) d.inject[tb + t.ix + at], 0), n - 1);
            z = d.inject[tb + t.z + at];
        } else {
            k = (int) mayfly_perm((uint32_t) q, c.kb_n, (uint32_t) n, c.seed, 2u + (uint32_t) u, gen,
                    stream_word(STREAM_MAYFLY_PERM, (uint32_t) (c.sub0 + p)));
            double z1;
            normal_pair(c.seed, (uint32_t) q, (uint32_t) u, gen, stream_word(STREAM_MAYFLY_Z, (uint32_t) (c.sub0 + p)), z, z1);
        }
        if (d.draws) {
            d.draws[tb + t.ix + at] = (double) k;
            d.draws[tb + t.z + at] = z;
        }
        const double sg = c.sigma * (d.upper[k] - d.lower[k]);
        o[k] = mayfly_clamp(px[k] + sg * z, d.lower[k], d.upper[k]);
    }
    if (c.obj != OBJ_HOST) {
        const double f = mayfly_value(d, c, o, lane);
        if (lane == 0) d.Uf[(size_t) p * c.nmut + u] = f;
    }
}

// the record t of a selection (fem 0: the males', 1: the females'): t < np the swarm's own fly of rank t,
// then half the shuffled offspring, then half the shuffled mutated flies.  Returns the kind (0 swarm,
// 1 offspring, 2 mutated) and the row of that kind.
__device__ inline int mayfly_record(const MayflyDev &d, const MayflyConst &c, int p, int fem, int t, int &row)
{
    const int np = c.np, h = np / 2, hm = c.nmut / 2;
    if (t < np) {
        row = min(max((fem ? d.ordf : d.ordm)[(size_t) p * np + t], 0), np - 1);
        return 0;
    }
    if (t < np + h) {
        row = min(max(d.permo[(size_t) p * np + (fem ? h : 0) + (t - np)], 0), np - 1);
        return 1;
    }
    row = min(max(d.permu[(size_t) p * c.nmut + (fem ? hm : 0) + (t - np - h)], 0), c.nmut - 1);
    return 2;
}

// :213-219 and :232-236: the first of the least values of offspring 0 .. np - 1 and mutated flies 0 .. nmut - 1
// takes fbest when it is below it; then the values the two selections sort.  grid (P), 256 threads
__global__ __launch_bounds__(256) void mayfly_merge(MayflyDev d, MayflyConst c)
{
    __shared__ double sval[4];
    __shared__ int sidx[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    MayflyScal *sc = d.scal + p;
    if (!sc->active) return;
    const int np = c.np, nmut = c.nmut;
    const double fbest = sc->fbest;
    __syncthreads();
    double v = MAYFLY_INF;
    int at = 0x7fffffff;
    for (int t = tid; t < np + nmut; t += 256) {
        const double f = t < np ? d.Of[(size_t) p * np + t] : d.Uf[(size_t) p * nmut + (t - np)];
        if (f < v) {
            v = f;
            at = t;
        }
    }
    block_arg<1>(v, at, sval, sidx);
    if (v < fbest) {
        const double *x = at < np ? d.OX + ((size_t) p * np + at) * c.ld : d.UX + ((size_t) p * nmut + (at - np)) * c.ld;
        for (int i = tid; i < c.n; i += 256) d.best[(size_t) p * c.ld + i] = x[i];
        if (tid == 0) {
            sc->fbest = v;
            sc->took = 2 * np + at;
        }
    }
    for (int q = tid; q < 2 * c.cm; q += 256) {
        const int fem = q >= c.cm ? 1 : 0, t = q - fem * c.cm;
        int row;
        const int kind = mayfly_record(d, c, p, fem, t, row);
        double f;
        if (kind == 0) f = (fem ? d.Ff : d.Mf)[(size_t) p * np + row];
        else if (kind == 1) f = d.Of[(size_t) p * np + row];
        else f = d.Uf[(size_t) p * nmut + row];
        d.keys[((size_t) p * 2 + fem) * c.cm + t] = f;
    }
}

// :250-258 / :269-275 without moving a row.  The reference copies record T[j] into slot j for j = 0, 1, ...
// while T still points at the swarm's own objects: a fly of rank k stands at T[j] only for j >= k (the
// swarm is sorted and the order stable), and for j > k it holds what landed in slot k.  So the record that
// lands in slot j is src[j] = T[j] is the swarm's fly k < j ? src[k] : T[j], a chain over integers that one
// lane walks in LDS.  repair: src[j] = T[j].  Then the schedule (:277-281) and the budget.
// grid (P), 128 threads: a wavefront per swarm
__global__ __launch_bounds__(128) void mayfly_resolve(MayflyDev d, MayflyConst c)
{
#pragma clang fp contract(off)
    __shared__ int src[2][MAYFLY_MAX_NP];
    const int p = blockIdx.x, lane = threadIdx.x & 63, fem = threadIdx.x >> 6;
    MayflyScal *sc = d.scal + p;
    if (!sc->active) return;
    const int np = c.np;
    const int *T = d.ordt + ((size_t) p * 2 + fem) * c.cm;
    for (int j = lane; j < np; j += 64) src[fem][j] = min(max(T[j], 0), c.cm - 1);
    wave_sync();
    if (lane == 0 && !c.repair)
        for (int j = 0; j < np; j++) {
            const int t = src[fem][j];
            if (t < j) src[fem][j] = src[fem][t];
        }
    wave_sync();
    int *out = (fem ? d.srcf : d.srcm) + (size_t) p * np;
    for (int j = lane; j < np; j += 64) out[j] = src[fem][j];
    if (threadIdx.x == 0) {
        MayflyScal s = *sc;
        s.fev += 3 * np + c.nmut;
        s.it++;
        s.g = c.gmax - ((c.gmax - c.gmin) / s.itmax) * s.it;
        s.dance *= c.ddamp;
        s.fl *= c.fldamp;
        if (!s.stop && s.fev >= c.mfev) s.stop = 2;
        *sc = s;
    }
}

// The selected records into the other buffer, slot by slot; a population whose generation did not run keeps
// its rows.  blockIdx.z: 0 males (x, v, bx, f, bf), 1 females (x, v, f).  grid (np, P, 2), 64 threads
__global__ __launch_bounds__(64) void mayfly_copy(MayflyDev d, MayflyConst c)
{
    const int j = blockIdx.x, p = blockIdx.y, fem = blockIdx.z, lane = threadIdx.x;
    const int np = c.np, ld = c.ld;
    int kind = 0, row = j;
    if (d.scal[p].active) {
        const int t = min(max((fem ? d.srcf : d.srcm)[(size_t) p * np + j], 0), c.cm - 1);
        kind = mayfly_record(d, c, p, fem, t, row);
    }
    const size_t dst = ((size_t) p * np + j) * ld, dsf = (size_t) p * np + j;
    const size_t srs = (size_t) p * np + row;
    const double *x = kind == 0 ? (fem ? d.FX : d.MX) + srs * ld : kind == 1 ? d.OX + srs * ld
            : d.UX + ((size_t) p * c.nmut + row) * ld;
    const double *v = kind == 0 ? (fem ? d.FV : d.MV) + srs * ld : nullptr;
    const double *bx = kind == 0 && !fem ? d.MBX + srs * ld : x;
    const double f = kind == 0 ? (fem ? d.Ff : d.Mf)[srs] : kind == 1 ? d.Of[srs] : d.Uf[(size_t) p * c.nmut + row];
    const double bf = kind == 0 && !fem ? d.Mbf[srs] : f;
    for (int i = lane; i < ld; i += 64) {
        const double xi = x[i], vi = v ? v[i] : 0.;
        if (fem) {
            d.FX2[dst + i] = xi;
            d.FV2[dst + i] = vi;
        } else {
            d.MX2[dst + i] = xi;
            d.MV2[dst + i] = vi;
            d.MBX2[dst + i] = bx[i];
        }
    }
    if (lane == 0) {
        if (fem) {
            d.Ff2[dsf] = f;
        } else {
            d.Mf2[dsf] = f;
            d.Mbf2[dsf] = bf;
        }
    }
}

} // namespace bbo
