// bbo_pikaia_kernels.hpp -- PIKAIA as gfx950 kernels.
//
//   kernel          reference lines (pikaia.cpp)                                     work per population
//   pikaia_init     :57-63 uniform phenotypes, mapped, and their values              np rows
//   pikaia_breed    :75-99 select, encode, cross, mutate, decode, genrep, and the
//                   value of both children where the objective is built in           np / 2 matings, a wavefront each
//   pikaia_newpop   :574-578 the elite test and copy; :586-591 fitness and ranking;
//                   :408-434 adjmut; :465 the running sums of select; counters, stop np values, one workgroup
//   pikaia_copy     :583 the new population becomes the old                          np rows
#pragma once

#include "bbo_pikaia.hpp"
#include "bbo_objectives.hpp"
#include "bbo_rank.hpp"
#include "bbo_rng.hpp"
#include "bbo_wave.hpp"

namespace bbo {

#define PIKAIA_INF (__builtin_huge_val())

// The draw table of one generation and population (bbo_pikaia_inject_draws, "draws"), in doubles: np / 2
// matings of `per_mating` values each,
//   [0]                 the uniform of the first parent
//   [1, 1 + ATTEMPTS)   the uniforms of the second parent, one per attempt (-1 behind the one that stood)
//   [x, x + 4)          cross: the coin against pcross, ispl, the coin one- / two-point, ispl2
//   child 0, child 1    each: the coin creep / uniform (imut >= 4), n nd locus uniforms, n nd value uniforms
//                       (the new digit int(10 u), or the creep step round(u) 2 - 1)
// -1 wherever the reference draws nothing.
struct PikaiaTable {
    int p2, x, child, per_child, loci, per_mating;
    size_t len;
};

__host__ __device__ inline PikaiaTable pikaia_table(int n, int np, int nd)
{
    PikaiaTable t;
    t.p2 = 1;
    t.x = 1 + PIKAIA_ATTEMPTS;
    t.child = t.x + 4;
    t.loci = n * nd;
    t.per_child = 1 + 2 * t.loci;
    t.per_mating = t.child + 2 * t.per_child;
    t.len = (size_t) (np / 2) * t.per_mating;
    return t;
}

static __device__ const int PIKAIA_P10[10] = { 1, 10, 100, 1000, 10000, 100000, 1000000, 10000000, 100000000,
        1000000000 };

// the fitness the GA maximises: -f, or f itself under raw; NaN ranks worst.  An objective program's NaN
// arrives as +inf (its evaluation kernels store NaN last for the minimising engines, bbo_program.hip), which
// under raw would rank best: there a +inf from a program ranks worst too.
__device__ inline double pikaia_fitness(const PikaiaConst &c, double f)
{
    if (c.raw && c.prog && f == PIKAIA_INF) return -PIKAIA_INF;
    const double v = c.raw ? f : -f;
    return v != v ? -PIKAIA_INF : v;
}

// x = lower + u (upper - lower), one multiply and one add; raw: u itself
__device__ inline double pikaia_map(const PikaiaDev &d, const PikaiaConst &c, int i, double u)
{
#pragma clang fp contract(off)
    if (c.raw) return u;
    const double w = d.upper[i] - d.lower[i];
    const double s = u * w;
    return d.lower[i] + s;
}

// A draw of the mating itself (the same in every lane: the scalar unit computes it): slot s of mating m.
// `at`: its place in the table.
__device__ inline double pikaia_mating_draw(const PikaiaDev &d, const PikaiaConst &c, int p, int m, uint32_t gen,
        int slot, size_t at, int lane)
{
    double u;
    if (d.inject) {
        u = d.inject[at];
    } else {
        const u32x4 w = philox4x32_10_uniform(c.seed, (uint32_t) slot >> 1, (uint32_t) m, gen,
                stream_word(STREAM_PIKAIA_MATE, (uint32_t) (c.sub0 + p)));
        u = (slot & 1) ? u01(w.z, w.w) : u01(w.x, w.y);
    }
    if (d.draws && lane == 0) d.draws[at] = u;
    return u;
}

// :460-472 by bisection over the running sums: the first row whose sum reaches the dice (row np - 1 when
// rounding leaves every sum below it)
__device__ inline int pikaia_select(const double *cum, int np, double u)
{
#pragma clang fp contract(off)
    const double dice = u * np * (np + 1);
    int lo = 0, hi = np - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] >= dice) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the uniforms of four loci (digits 4 q .. 4 q + 3 of gene i, child ch): one 32-bit word each
__device__ inline void pikaia_locus_words(const PikaiaConst &c, int p, int m, int ch, int i, int q, int purpose,
        uint32_t gen, double (&u)[4])
{
    const u32x4 w = philox4x32_10(c.seed, (uint32_t) i | ((uint32_t) q << 12),
            (uint32_t) m | ((uint32_t) ch << 12) | ((uint32_t) purpose << 16), gen,
            stream_word(STREAM_PIKAIA_LOCUS, (uint32_t) (c.sub0 + p)));
    u[0] = (double) w.x * 0x1.0p-32;
    u[1] = (double) w.y * 0x1.0p-32;
    u[2] = (double) w.z * 0x1.0p-32;
    u[3] = (double) w.w * 0x1.0p-32;
}

// :330-406 for gene i of child ch, the gene as the integer v its nd digits spell.  Digit j (0: the most
// significant) weighs pw = 10^(nd - 1 - j).  Creep: +1 carries into the digits above exactly as v + pw does;
// when they are all 9 the reference sets digits 0 .. j to 9 and leaves the rest: zi - pw + v mod pw.  -1
// borrows as v - pw does; when the digits 0 .. j are all 0 (v < pw) they stay 0: v itself.
// tc: the child's place in the table.
__device__ inline int pikaia_mutate_gene(const PikaiaDev &d, const PikaiaConst &c, int p, int m, int ch, int i,
        uint32_t gen, bool creep, double pmut, int v, size_t tc)
{
#pragma clang fp contract(off)
    const int nd = c.nd, loci = c.n * nd;
    const size_t tl = tc + 1 + (size_t) i * nd, tv = tl + loci;
    for (int q = 0; 4 * q < nd; q++) {
        double ul[4], uv[4];
        bool have_v = false;
        if (!d.inject) pikaia_locus_words(c, p, m, ch, i, q, 1, gen, ul);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int j = 4 * q + t;
            if (j >= nd) break;
            const double u = d.inject ? d.inject[tl + j] : ul[t];
            if (d.draws) d.draws[tl + j] = u;
            if (!(u < pmut)) continue;
            double w;
            if (d.inject) {
                w = d.inject[tv + j];
            } else {
                if (!have_v) pikaia_locus_words(c, p, m, ch, i, q, 2, gen, uv);
                have_v = true;
                w = uv[t];
            }
            if (d.draws) d.draws[tv + j] = w;
            const int pw = PIKAIA_P10[nd - 1 - j];
            if (creep) {
                if (w >= 0.5) v = v + pw < c.zi ? v + pw : c.zi - pw + v % pw;      // round(w) 2 - 1 = +1
                else v = v >= pw ? v - pw : v;
            } else {
                const int nw = (int) (w * 10.), old = (v / pw) % 10;
                v += (nw - old) * pw;
            }
        }
    }
    return v;
}

// :57-63: row r of population p, a wavefront per row, into the NEW buffers (pikaia_newpop and pikaia_copy make
// them the population).  grid (np, P), 64 threads
__global__ __launch_bounds__(64) void pikaia_init(PikaiaDev d, PikaiaConst c)
{
#pragma clang fp contract(off)
    const int r = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
    const size_t row = ((size_t) p * c.np + r) * c.ld;
    for (int i = lane; i < c.ld; i += 64) {
        double u = 0., x = 0.;
        if (i < c.n) {
            const u32x4 w = philox4x32_10(c.seed, (uint32_t) r, (uint32_t) i, 0,
                    stream_word(STREAM_PIKAIA_INIT, (uint32_t) (c.sub0 + p)));
            u = u01(w.x, w.y);
            x = pikaia_map(d, c, i, u);
        }
        d.newph[row + i] = u;
        d.newx[row + i] = x;
    }
    if (c.obj != OBJ_HOST) {
        wave_sync();
        const double f = eval_row_group<64>(c.obj, c.n, d.newx + row, d.aux, lane);
        if (lane == 0) d.newf[(size_t) p * c.np + r] = f;
    }
}

// Mating m of population p (:75-99).  The draws of the mating are computed by every lane (no broadcast), a
// lane owns coordinate i, i + 64, ... of both children.  grid (np / 2, P), 64 threads
__global__ __launch_bounds__(64) void pikaia_breed(PikaiaDev d, PikaiaConst c)
{
#pragma clang fp contract(off)
    const int m = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
    const PikaiaScal *sc = d.scal + p;
    if (pop_frozen(c, sc)) return;
    const int n = c.n, np = c.np, nd = c.nd, ld = c.ld;
    const PikaiaTable t = pikaia_table(n, np, nd);
    const size_t tb = (size_t) p * c.table + (size_t) m * t.per_mating;
    if (d.draws) {
        for (int q = lane; q < t.per_mating; q += 64) d.draws[tb + q] = -1.;
        wave_sync();
    }
    const double *cum = d.cum + (size_t) p * np;
    const double pmut = sc->pmut;
    const uint32_t gen = (uint32_t) sc->ig;

    // 1. the parents (:78-82)
    const int ip1 = pikaia_select(cum, np, pikaia_mating_draw(d, c, p, m, gen, 0, tb, lane));
    int ip2 = ip1;
    for (int a = 0; a < PIKAIA_ATTEMPTS; a++) {
        const double u = pikaia_mating_draw(d, c, p, m, gen, t.p2 + a, tb + t.p2 + a, lane);
        if (u < 0.) break;      // (an injected table that ends here)
        ip2 = pikaia_select(cum, np, u);
        if (ip2 != ip1) break;
    }
    if (ip2 == ip1) ip2 = ip1 + 1 < np ? ip1 + 1 : 0;

    // 3a. the crossover window (:301-319), loci 1-based
    int ispl = -1, ispl2 = -1;
    if (pikaia_mating_draw(d, c, p, m, gen, t.x, tb + t.x, lane) < c.pcross) {
        ispl = (int) (pikaia_mating_draw(d, c, p, m, gen, t.x + 1, tb + t.x + 1, lane) * n * nd) + 1;
        if (pikaia_mating_draw(d, c, p, m, gen, t.x + 2, tb + t.x + 2, lane) < 0.5) {
            ispl2 = n * nd;
        } else {
            ispl2 = (int) (pikaia_mating_draw(d, c, p, m, gen, t.x + 3, tb + t.x + 3, lane) * n * nd) + 1;
            if (ispl2 < ispl) {
                const int tmp = ispl2;
                ispl2 = ispl;
                ispl = tmp;
            }
        }
    }
    // 3b. the kind of mutation per child (:334)
    bool creep[2] = { false, false };
    if (c.imut >= 4) {
#pragma unroll
        for (int ch = 0; ch < 2; ch++)
            creep[ch] = pikaia_mating_draw(d, c, p, m, gen, t.child + ch, tb + t.child + (size_t) ch * t.per_child,
                    lane) <= 0.5;
    }
    if (lane == 0) {
        d.parents[((size_t) p * (np / 2) + m) * 2] = ip1;
        d.parents[((size_t) p * (np / 2) + m) * 2 + 1] = ip2;
        d.cross[((size_t) p * (np / 2) + m) * 2] = ispl;
        d.cross[((size_t) p * (np / 2) + m) * 2 + 1] = ispl2;
        d.mode[(size_t) p * np + 2 * m] = creep[0] ? 1 : 0;
        d.mode[(size_t) p * np + 2 * m + 1] = creep[1] ? 1 : 0;
    }

    const double *ph1 = d.ph + ((size_t) p * np + ip1) * ld, *ph2 = d.ph + ((size_t) p * np + ip2) * ld;
    const size_t r1 = ((size_t) p * np + 2 * m) * ld, r2 = r1 + ld;
    for (int i = lane; i < ld; i += 64) {
        double u1 = 0., u2 = 0., x1 = 0., x2 = 0.;
        if (i < n) {
            // 2. encode (:276-280): the nd digits the reference keeps are ip mod 10^nd
            int v1 = (int) (ph1[i] * c.z) % c.zi, v2 = (int) (ph2[i] * c.z) % c.zi;
            // 3c. the digits of this gene inside the window change sides (:322-326)
            const int lo = max(ispl, i * nd + 1), hi = min(ispl2, i * nd + nd);
            if (ispl > 0 && lo <= hi) {
                const int a = lo - 1 - i * nd, b = hi - 1 - i * nd;
                const int lowp = PIKAIA_P10[nd - 1 - b], span = PIKAIA_P10[b - a + 1];
                const int m1 = (v1 / lowp) % span, m2 = (v2 / lowp) % span;
                v1 += (m2 - m1) * lowp;
                v2 += (m1 - m2) * lowp;
            }
            v1 = pikaia_mutate_gene(d, c, p, m, 0, i, gen, creep[0], pmut, v1, tb + t.child);
            v2 = pikaia_mutate_gene(d, c, p, m, 1, i, gen, creep[1], pmut, v2, tb + t.child + t.per_child);
            // 4. decode (:289-293) and map
            u1 = v1 * c.zinv;
            u2 = v2 * c.zinv;
            x1 = pikaia_map(d, c, i, u1);
            x2 = pikaia_map(d, c, i, u2);
        }
        d.newph[r1 + i] = u1;
        d.newph[r2 + i] = u2;
        d.newx[r1 + i] = x1;
        d.newx[r2 + i] = x2;
    }
    if (c.obj != OBJ_HOST) {
        wave_sync();
        const double f1 = eval_row_group<64>(c.obj, n, d.newx + r1, d.aux, lane);
        const double f2 = eval_row_group<64>(c.obj, n, d.newx + r2, d.aux, lane);
        if (lane == 0) {
            d.newf[(size_t) p * np + 2 * m] = f1;
            d.newf[(size_t) p * np + 2 * m + 1] = f2;
        }
    }
}

// newpop, adjmut and what select needs, one workgroup per population; `mode`: PikaiaNewpopMode.
// grid (P), sort_threads(m) threads, 12 max(m, 1024) bytes of LDS (m = rank_sort_m(np))
__global__ __launch_bounds__(1024) void pikaia_newpop(PikaiaDev d, PikaiaConst c, int mode, int m)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double sortbuf[];
    __shared__ int took;     // the row that took fbest (-1: none)
    const int p = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    PikaiaScal *sc = d.scal + p;
    const bool init = (mode & PIKAIA_INIT) != 0;
    if (!init && pop_frozen(c, sc)) {
        if (tid == 0 && (mode & PIKAIA_REST)) sc->active = 0;
        return;
    }
    const int np = c.np, n = c.n, ld = c.ld;
    double *fitns = d.fitns + (size_t) p * np, *newf = d.newf + (size_t) p * np;
    int *order = d.order + (size_t) p * np, *rank = d.rank + (size_t) p * np;
    double *newph = d.newph + (size_t) p * np * ld, *newx = d.newx + (size_t) p * np * ld;

    // :574-578: the value of new row 0 against the stored value of the old best
    if ((mode & PIKAIA_ELITE) && c.ielite && !init) {
        const int ib = min(max(order[np - 1], 0), np - 1);
        const double fold = fitns[ib];
        const bool take = pikaia_fitness(c, newf[0]) < fold;
        __syncthreads();
        if (take) {
            const double *oph = d.ph + ((size_t) p * np + ib) * ld, *ox = d.x + ((size_t) p * np + ib) * ld;
            for (int i = tid; i < ld; i += T) {
                newph[i] = oph[i];
                newx[i] = ox[i];
            }
            __syncthreads();
            // its value: what the objective returns for it (a host objective or a program follows this
            // launch); repair: the stored one
            if (c.repair) {
                if (tid == 0) newf[0] = c.raw ? fold : -fold;
            } else if (c.obj != OBJ_HOST && tid < 64) {
                const double f = eval_row_group<64>(c.obj, n, newx, d.aux, tid);
                if (tid == 0) newf[0] = f;
            }
        }
        if (tid == 0) sc->elite = take ? 1 : 0;
        __syncthreads();
    }
    if (!(mode & (PIKAIA_REST | PIKAIA_INIT))) return;

    // :586: the fitness of every row (init, :62: the value of the last row in the last slot, the rest 0)
    for (int r = tid; r < np; r += T) {
        double f = pikaia_fitness(c, newf[r]);
        if (init && !c.repair && r != np - 1) f = 0.;
        fitns[r] = f;
    }
    __syncthreads();
    double *keys = sortbuf;
    int *idx = reinterpret_cast<int*>(sortbuf + max(m, 1024));
    bitonic_sort_lds(fitns, np, m, keys, idx, order, rank);
    __syncthreads();

    // the weights of select (:465) by row, then their running sums from left to right
    double *wts = sortbuf;
    for (int r = tid; r < np; r += T) wts[r] = c.fdif * (np + 1 - 2 * (np - rank[r]));
    __syncthreads();
    if (tid == 0) {
        double rt = 0.;
        for (int r = 0; r < np; r++) {
            rt = rt + (np + 1) + wts[r];
            wts[r] = rt;
        }
    }
    __syncthreads();
    for (int r = tid; r < np; r += T) d.cum[(size_t) p * np + r] = wts[r];

    if (tid == 0) {
        PikaiaScal s = *sc;
        const int ib = order[np - 1], im = order[np / 2 - 1];
        // the best ever (init without repair ranks placeholders: the values themselves are scanned)
        int jb = ib;
        double fb = fitns[ib];
        if (init && !c.repair) {
            fb = -PIKAIA_INF;
            jb = 0;
            for (int r = 0; r < np; r++) {
                const double f = pikaia_fitness(c, newf[r]);
                if (f > fb) {
                    fb = f;
                    jb = r;
                }
            }
        }
        took = -1;
        if (init || fb > s.fbest) {
            s.fbest = fb;
            took = jb;
        }
        if (init) {
            s.fev = np;
            s.ig = 1;
            s.rdif = 0.;
            s.elite = 0;
        } else {
            // :408-434
            if (c.imut == 2 || c.imut == 3 || c.imut == 5 || c.imut == 6) {
                double rdif;
                if (c.imut == 2 || c.imut == 5) {
                    const double a = fitns[ib], b = fitns[im];
                    const double den = a + b;
                    rdif = fabs(a - b) / (c.repair ? fabs(den) : den);
                } else {
                    rdif = 0.;
                    const double *xa = newph + (size_t) ib * ld, *xb = newph + (size_t) im * ld;
                    for (int i = 0; i < n; i++) {
                        const double dd = xa[i] - xb[i];
                        rdif += dd * dd;
                    }
                    rdif = sqrt(rdif) / n;
                }
                s.rdif = rdif;
                if (rdif <= 0.05) {
                    const double v = s.pmut * 1.5;
                    s.pmut = c.pmutmx < v ? c.pmutmx : v;
                } else if (rdif >= 0.25) {
                    const double v = s.pmut / 1.5;
                    s.pmut = c.pmutmn < v ? v : c.pmutmn;
                }
            }
            if (!c.ielite) s.elite = 0;
            s.fev += c.repair ? np : np + 1;    // :579, :588
            s.ig++;
        }
        if (s.ig > c.ngen) {
            s.stop = 1;
            s.conv = 1;
        }
        s.active = 1;
        *sc = s;
    }
    __syncthreads();
    if (took >= 0)
        for (int i = tid; i < ld; i += T) d.best[(size_t) p * ld + i] = newx[(size_t) took * ld + i];
}

// :583: the new population becomes the old one.  grid (np, P), 64 threads
__global__ __launch_bounds__(64) void pikaia_copy(PikaiaDev d, PikaiaConst c)
{
    const int r = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
    if (!d.scal[p].active) return;
    const size_t row = ((size_t) p * c.np + r) * c.ld;
    for (int i = lane; i < c.ld; i += 64) {
        d.ph[row + i] = d.newph[row + i];
        d.x[row + i] = d.newx[row + i];
    }
}

} // namespace bbo
