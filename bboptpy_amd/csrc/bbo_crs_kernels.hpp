// bbo_crs_kernels.hpp -- CRS as gfx950 kernels.
//
//   kernel       reference lines (crs.cpp)                                    work per population
//   crs_init     :61-70 uniform points and their values                       np rows
//   crs_rank     :78 the sorted pool, as order[rank] = row (stable)           np values
//   crs_eval     :135, :146 the value of the pending point                    one row
//   crs_steps    :111-166 trial() as a resumable state machine, update()      a bounded number of steps
#pragma once

#include "bbo_crs.hpp"
#include "bbo_objectives.hpp"
#include "bbo_rank.hpp"
#include "bbo_rng.hpp"
#include "bbo_wave.hpp"

namespace bbo {

#define CRS_INF (__builtin_huge_val())

enum CrsInitMode { CRS_INIT_DRAW = 1, CRS_INIT_EVAL = 2 };

constexpr int CRS_INIT_ROWS = 64;    // rows per workgroup of crs_init
constexpr int CRS_RANK_CANDS = 32;   // candidates per workgroup of crs_rank (rank_by_counting<8>)

// :61-70 for the populations p0 .. p0 + gridDim.x - 1, a wavefront per row; also what follows a set of
// "x".  Random::get(lower, upper) on doubles over the raw uniform (random.hpp:329-337).
// grid (populations, ceil(np / CRS_INIT_ROWS)), 256 threads
__global__ __launch_bounds__(256) void crs_init(CrsDev d, CrsConst c, int p0, int mode)
{
#pragma clang fp contract(off)
    const int p = p0 + blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = c.n, np = c.np;
    const int r1 = min(np, ((int) blockIdx.y + 1) * CRS_INIT_ROWS);
    for (int r = blockIdx.y * CRS_INIT_ROWS + wave; r < r1; r += 4) {
        double *x = d.X + ((size_t) p * np + r) * c.ld;
        if (mode & CRS_INIT_DRAW) {
            for (int j = lane; j < c.ld; j += 64) {
                double v = 0.;
                if (j < n) {
                    const u32x4 w = philox4x32_10(c.seed, (uint32_t) r, (uint32_t) j, 0,
                            stream_word(STREAM_CRS_INIT, (uint32_t) p));
                    const double a = d.lower[j], b = d.upper[j];
                    const double lo = a < b ? a : b, hi = a < b ? b : a;
                    v = u01(w.x, w.y) * (hi - lo) + lo;
                }
                x[j] = v;
            }
            wave_sync();
        }
        if (mode & CRS_INIT_EVAL) {
            double f = eval_row_group<64>(c.obj, n, x, d.aux, lane);
            if (f != f) f = CRS_INF;
            if (lane == 0) d.f[(size_t) p * np + r] = f;
        }
    }
}

// :78 without moving a row: order[rank of row] = row, equal values in row order (bbo_rank.hpp), and the
// best and the worst value.  grid (populations, ceil(np / CRS_RANK_CANDS)), 256 threads
__global__ __launch_bounds__(256) void crs_rank(CrsDev d, CrsConst c, int p0)
{
    __shared__ double tile[RANK_TILE];
    const int p = p0 + blockIdx.x, np = c.np;
    const double *f = d.f + (size_t) p * np;
    const int cand = blockIdx.y * CRS_RANK_CANDS + (threadIdx.x >> 3), slice = threadIdx.x & 7;
    const int r = rank_by_counting<8>(f, np, cand, slice, tile);
    if (cand < np && slice == 0) {
        d.order[(size_t) p * np + r] = cand;
        if (r == 0) d.scal[p].fbest = f[cand];
        if (r == np - 1) d.scal[p].fworst = f[cand];
    }
}

// :135 / :146 for a host-driven walk: the value of the pending point.  grid (P), 64 threads
__global__ __launch_bounds__(64) void crs_eval(CrsDev d, CrsConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    const CrsScal *sc = d.scal + p;
    if (!sc->pending || pop_frozen(c, sc)) return;
    const double *x = (sc->stage == CRS_WAIT_MUT ? d.cand2 : d.cand) + (size_t) p * c.ld;
    double f = eval_row_group<64>(c.obj, c.n, x, d.aux, threadIdx.x);
    if (f != f) f = CRS_INF;
    if (threadIdx.x == 0) d.value[p] = f;
}

// the hand-over point of crs_steps' T threads
template<int T>
__device__ inline void crs_sync()
{
    if (T == 64) wave_sync();
    else __syncthreads();
}

// `ok` in every thread of the workgroup, behind a hand-over point
template<int T>
__device__ inline bool crs_all(bool ok)
{
    if (T == 64) {
        wave_sync();
        return __all(ok) != 0;
    }
    return __syncthreads_and(ok) != 0;
}

// the value of the row x in LDS, in every thread: the first wavefront sums it (the sum crs_eval forms)
template<int T>
__device__ inline double crs_value(const CrsDev &d, const CrsConst &c, const double *x, double *slot)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    double v = 0.;
    if (tid < 64) {
        v = eval_row_group<64>(c.obj, c.n, x, d.aux, tid);
        if (v != v) v = CRS_INF;
        if (T > 64 && tid == 0) *slot = v;
    }
    if (T > 64) {
        __syncthreads();
        v = *slot;
        __syncthreads();
    }
    return v;
}

// The next record of draws: of the injected table (false: it is exhausted) and of the log.  Every
// thread keeps the same counters.
__device__ inline bool crs_next_record(const CrsDev &d, const CrsConst &c, CrsScal &s)
{
    if (d.inject) {
        if (s.irec >= c.inject_n) return false;
        s.irec++;
    }
    if (d.draws) s.nrec++;
    return true;
}

// the record the draws of the moment belong to: where the injected ones are read, where the log goes
__device__ inline const double* crs_record_in(const CrsDev &d, const CrsConst &c, const CrsScal &s, int p)
{
    return d.inject ? d.inject + ((size_t) p * c.inject_n + (s.irec - 1)) * 2 * c.n : nullptr;
}

__device__ inline double* crs_record_out(const CrsDev &d, const CrsConst &c, const CrsScal &s, int p)
{
    return d.draws && s.nrec <= c.record ? d.draws + ((size_t) p * c.record + (s.nrec - 1)) * 2 * c.n : nullptr;
}

// The hot path.  One workgroup of T threads per population; the lanes own the coordinates of t and t2 (in
// LDS for the launch, written back at its end), draw the n row indices of a trial together (one Philox
// call per four) and each walks its coordinate over the drawn rows in the reference's order, a division
// per term.  The first wavefront sums the objective from LDS.  Everything a later launch needs is in
// CrsScal, cand, cand2 and the bit stack.
//   mode   CRS_FUSED: evaluates inside; ends at the goal, at a stop or after c.launch_evals steps (then
//          *d.more is raised).  CRS_ADVANCE: ends where a point awaits its value.  CRS_ABSORB: takes
//          d.value[p] for the pending point, then advances.
//   begin  the goal becomes `it + K` first
// Draws: the indices of trial `trials` from (quad, 0, trials) of STREAM_CRS_IDX, the uniform of
// coordinate i of mutation `muts` from (i, 0, muts) of STREAM_CRS_W: keyed by what they are for, so a
// resumed launch draws nothing twice.
// LDS: t, t2, lower, upper [ld] each, then the n indices.  grid (P), T threads
template<int T>
__global__ __launch_bounds__(T) void crs_steps(CrsDev d, CrsConst c, int mode, int K, int begin)
{
#pragma clang fp contract(off)
    extern __shared__ double crs_lds[];
    __shared__ double bc_f;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = c.n, ld = c.ld, np = c.np;
    CrsScal s = d.scal[p];
    if (pop_frozen(c, &s)) return;
    if (mode == CRS_ABSORB && !s.pending) return;
    if (begin) s.goal = s.it + K;
    double *t = crs_lds, *t2 = t + ld, *lo = t2 + ld, *up = lo + ld;
    int *idx = reinterpret_cast<int*>(up + ld);
    double *X = d.X + (size_t) p * np * ld, *f = d.f + (size_t) p * np;
    int *ord = d.order + (size_t) p * np;
    uint32_t *stk = d.stack + (size_t) p * c.stack_words;
    for (int i = tid; i < n; i += T) {
        t[i] = d.cand[(size_t) p * ld + i];
        t2[i] = d.cand2[(size_t) p * ld + i];
        lo[i] = d.lower[i];
        up[i] = d.upper[i];
    }
    int rbest = ord[0], rworst = ord[np - 1];
    double fworst = f[rworst];
    const double dn = (double) n;
    const uint32_t sub = (uint32_t) p;
    int steps = 0;
    bool absorbed = false, more = false;
    crs_sync<T>();

    for (;;) {
        if (s.stage == CRS_IDLE) {
            if (s.it >= s.goal || (c.honor_stop && s.stop)) break;
            s.depth = 0;
            s.maxdepth = 0;
            s.nrec = 0;
            s.wused = 1;
            s.stage = CRS_CALL;
        }
        if (s.stage == CRS_CALL) {          // :114-134
            if (mode == CRS_FUSED && steps >= c.launch_evals) {
                more = true;
                break;
            }
            if (!crs_next_record(d, c, s)) {
                s.starved = 1;
                break;
            }
            s.wused = 0;
            const double *in = crs_record_in(d, c, s, p);
            double *out = crs_record_out(d, c, s, p);
            // (the reference indexes its SORTED pool: a drawn rank names the row order[rank])
            if (in) {
                for (int j = tid; j < n; j += T) {
                    const int r = min(max((int) in[j], 0), np - 1);
                    idx[j] = ord[r];
                    if (out) out[j] = (double) r;
                }
            } else {
                for (int q = tid; 4 * q < n; q += T) {
                    const u32x4 w = philox4x32_10(c.seed, (uint32_t) q, 0, (uint32_t) s.trials,
                            stream_word(STREAM_CRS_IDX, sub));
                    const uint32_t ws[4] = { w.x, w.y, w.z, w.w };
                    for (int e = 0; e < 4; e++) {
                        const int j = 4 * q + e;
                        if (j >= n) break;
                        const int r = uint_below(ws[e], np);
                        idx[j] = ord[r];
                        if (out) out[j] = (double) r;
                    }
                }
            }
            if (out)
                for (int j = tid; j < n; j += T) out[n + j] = 0.5;
            crs_sync<T>();
            bool inside = true;
            for (int i = tid; i < n; i += T) {
                double cc = 0.0;
                cc += X[(size_t) rbest * ld + i] / dn;
                // (eight rows are in flight together; the terms are still added in the reference's order)
                for (int j0 = 0; j0 < n - 1; j0 += 8) {
                    double v[8];
#pragma unroll
                    for (int e = 0; e < 8; e++) v[e] = j0 + e < n - 1 ? X[(size_t) idx[j0 + e] * ld + i] : 0.;
#pragma unroll
                    for (int e = 0; e < 8; e++)
                        if (j0 + e < n - 1) cc += v[e] / dn;
                }
                const double tv = 2 * cc - X[(size_t) idx[n - 1] * ld + i];
                t[i] = tv;
                if (tv < lo[i] || tv > up[i]) inside = false;
            }
            inside = crs_all<T>(inside);
            s.trials++;
            steps++;
            if (!inside) {
                if (s.depth >= c.max_depth) {       // (repair: redraws in a row without an evaluation)
                    s.stop = 3;
                    s.stage = CRS_IDLE;
                    s.depth = 0;
                    break;
                }
                if (!c.repair) {
                    if (tid == 0) stk[s.depth >> 5] &= ~(1u << (s.depth & 31));     // B
                    crs_sync<T>();
                }
                s.depth++;
                s.maxdepth = max(s.maxdepth, s.depth);
                continue;
            }
            if (c.repair) s.depth = 0;
            s.stage = CRS_WAIT_TRIAL;
            s.pending = 1;
        }
        if (s.stage == CRS_WAIT_TRIAL) {    // :135-147
            if (s.pending) {
                double v;
                if (mode == CRS_FUSED) {
                    if (steps >= c.launch_evals) {
                        more = true;
                        break;
                    }
                    steps++;
                    v = crs_value<T>(d, c, t, &bc_f);
                } else if (mode == CRS_ABSORB && !absorbed) {
                    v = d.value[p];
                    absorbed = true;
                } else {
                    break;
                }
                s.ft = v;
                s.fev++;
                s.pending = 0;
            }
            if (s.ft >= fworst) {
                if (s.wused && !crs_next_record(d, c, s)) {
                    s.starved = 1;
                    break;
                }
                const bool fresh = s.wused != 0;
                const double *in = crs_record_in(d, c, s, p);
                double *out = crs_record_out(d, c, s, p);
                for (int i = tid; i < n; i += T) {
                    double w;
                    if (in) {
                        w = in[n + i];
                    } else {
                        const u32x4 r = philox4x32_10(c.seed, (uint32_t) i, 0, (uint32_t) s.muts,
                                stream_word(STREAM_CRS_W, sub));
                        w = u01(r.x, r.y);
                    }
                    t2[i] = (1.0 + w) * X[(size_t) rbest * ld + i] - w * t[i];
                    if (out) {
                        if (fresh) out[i] = -1.;
                        out[n + i] = w;
                    }
                }
                s.wused = 1;
                s.muts++;
                crs_sync<T>();
                s.stage = CRS_WAIT_MUT;
                s.pending = 1;
            } else {
                s.stage = CRS_RET;
            }
        }
        if (s.stage == CRS_WAIT_MUT) {      // :146-156
            if (s.pending) {
                double v;
                if (mode == CRS_FUSED) {
                    if (steps >= c.launch_evals) {
                        more = true;
                        break;
                    }
                    steps++;
                    v = crs_value<T>(d, c, t2, &bc_f);
                } else if (mode == CRS_ABSORB && !absorbed) {
                    v = d.value[p];
                    absorbed = true;
                } else {
                    break;
                }
                s.ft2 = v;
                s.fev++;
                s.pending = 0;
            }
            if (s.ft2 >= fworst) {
                if (c.repair) {
                    if (s.fev >= c.mfev) {  // (the pair is redrawn: the budget is tested here too)
                        s.stop = 2;
                        s.stage = CRS_IDLE;
                        break;
                    }
                    s.stage = CRS_CALL;
                    continue;
                }
                if (s.depth >= c.max_depth) {
                    s.stop = 3;
                    s.stage = CRS_IDLE;
                    s.depth = 0;
                    break;
                }
                if (tid == 0) stk[s.depth >> 5] |= 1u << (s.depth & 31);    // M
                crs_sync<T>();
                s.depth++;
                s.maxdepth = max(s.maxdepth, s.depth);
                s.stage = CRS_CALL;
                continue;
            }
            s.ft = s.ft2;
            for (int i = tid; i < n; i += T) t[i] = t2[i];
            crs_sync<T>();
            s.stage = CRS_RET;
        }
        if (s.stage == CRS_RET) {
            bool again = false;
            while (s.depth > 0) {
                s.depth--;
                if (((stk[s.depth >> 5] >> (s.depth & 31)) & 1u) == 0) {    // B: back to :135
                    s.stage = CRS_WAIT_TRIAL;
                    s.pending = 1;
                    again = true;
                    break;
                }
                s.ft = s.ft2;                                               // M: :155-156
                for (int i = tid; i < n; i += T) t[i] = t2[i];
                crs_sync<T>();
            }
            if (again) continue;
            // update() (:160-166): the point into the worst's row, the row to its rank behind the
            // values that are <= its own
            const int row = rworst;
            if (s.ft >= fworst) s.stale++;
            for (int i = tid; i < n; i += T) X[(size_t) row * ld + i] = t[i];
            if (tid == 0) f[row] = s.ft;
            int a = 0, b = np - 1;
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (f[ord[mid]] <= s.ft) a = mid + 1;
                else b = mid;
            }
            const int slot = a;
            for (int hi = np - 1; hi > slot; hi -= T) {
                const int i = hi - tid;
                int v = 0;
                if (i > slot) v = ord[i - 1];
                crs_sync<T>();
                if (i > slot) ord[i] = v;
                crs_sync<T>();
            }
            if (tid == 0) ord[slot] = row;
            crs_sync<T>();
            rbest = ord[0];
            rworst = ord[np - 1];
            fworst = f[rworst];
            s.fbest = f[rbest];
            s.fworst = fworst;
            s.it++;
            s.stage = CRS_IDLE;
            s.conv = fabs(s.fbest - s.fworst) < c.tol ? 1 : 0;      // :168-172
            if (!s.stop) {
                if (s.conv) s.stop = 1;
                else if (s.fev >= c.mfev) s.stop = 2;
            }
        }
    }

    for (int i = tid; i < n; i += T) {
        d.cand[(size_t) p * ld + i] = t[i];
        d.cand2[(size_t) p * ld + i] = t2[i];
    }
    if (tid == 0) {
        d.scal[p] = s;
        if (more) *d.more = 1;
    }
}

} // namespace bbo
