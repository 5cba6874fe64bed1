// bbo_nm_kernels.hpp -- NelderMead as gfx950 kernels.
//
//   kernel    reference lines (nelder_mead.cpp)                               work per population
//   nm_walk   :89-226 iterate(), :245-304 nelmin(), :312-367 initSimplex()    steps of 1, 2 or n + 1 evaluations
//   nm_eval   the values of a pending batch with a built-in (bbo_nm_phase 1)   up to 2 n rows
//
// Lane i owns coordinate i: the centroid (its fold over the n + 1 rows in row order, less row ihi, divided
// by n), the reflection, the expansion, both contractions, the copy into row ihi, the shrink (in place, row
// after row, reading row ilo as it stands) and the probes of the factorial test.  ihi, ilo, l and the stop
// test's two sums are the reference's sequential folds over y in LDS, the same in every lane.  Nothing is
// contracted into a fused multiply-add.
#pragma once

#include "bbo_nm.hpp"
#include "bbo_objectives.hpp"
#include "bbo_rng.hpp"
#include "bbo_wave.hpp"

namespace bbo {

#define NM_INF (__builtin_huge_val())

// a built-in at one row, by one wavefront; a NaN counts as +inf
__device__ inline double nm_value(const NmConst &c, const double *row, const double *aux, int lane)
{
    const double f = eval_row_group<64>(c.obj, c.n, row, aux, lane);
    return f != f ? NM_INF : f;
}

#ifndef BBO_WALK_DEVICE_FUNCTIONS_ONLY   // (bbo_bh.hip takes the value function and the re-arm, not the kernels)
// grid (P), 64 threads (n <= 64) or 128; dynamic LDS: the simplex, (n + 1) ld doubles, under c.lds
//   mode   NM_FUSED: evaluates inside and ends at the goal or a stop.  NM_ADVANCE: walks to the next batch
//          of points, leaves them in `cand` (or in the simplex: a fresh or a shrunk one) and ends.
//          NM_ABSORB: takes d.value for the pending batch, then advances.
//   begin  the goal becomes `it + K` first
// c.honor_stop (bbo_run) makes the walk nelmin(): the factorial test, restarts and the two stops.
__global__ __launch_bounds__(NM_THREADS) void nm_walk(NmDev d, NmConst c, int mode, int K, int begin)
{
#pragma clang fp contract(off)
    extern __shared__ double nm_simplex[];
    __shared__ double ys[NM_MAX_N + 2], vals[2 * NM_MAX_N];
    __shared__ double pbar[NM_MAX_N], pstar[NM_MAX_N], p2star[NM_MAX_N];
    __shared__ double xm[NM_MAX_N], fa[NM_MAX_N], fb[NM_MAX_N], fd[NM_MAX_N];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nt = blockDim.x, nw = nt >> 6;
    const int n = c.n, ld = c.ld, n1 = n + 1;
    NmScal s = d.scal[p];
    if (pop_frozen(c, &s)) return;
    if (mode == NM_ABSORB && !s.pending) return;
    if (mode == NM_ADVANCE && s.pending) return;
    if (begin) s.goal = s.it + K;
    if (s.stage == NM_IDLE && s.it >= s.goal && !(c.honor_stop && (s.conv || s.fev >= c.mfev))) return;

    const size_t pv = (size_t) p * ld;
    double *G = d.P + (size_t) p * n1 * ld;
    double *S = c.lds ? nm_simplex : G;
    double *cand = d.cand + (size_t) p * 2 * n * ld;
    const double *val = d.value + (size_t) p * c.vs;
    const double *step = d.step + pv;
    if (c.lds)
        for (int q = tid; q < n1 * ld; q += nt) S[q] = G[q];
    for (int q = tid; q < n1; q += nt) ys[q] = d.y[(size_t) p * n1 + q];
    const bool absorb = mode == NM_ABSORB;
    if (absorb) {
        for (int q = tid; q < s.pending; q += nt) vals[q] = val[q];
        if (tid < n) {
            pstar[tid] = cand[tid];
            p2star[tid] = cand[ld + tid];
            xm[tid] = d.xmin[pv + tid];
        }
        s.pending = 0;
    }
    __syncthreads();

    // :96-106, lane i its coordinate
    auto centroid = [&] {
        if (tid < n) {
            double sum = 0.;
            for (int k = 0; k < n1; k++) sum += S[(size_t) k * ld + tid];
            sum -= S[(size_t) s.ihi * ld + tid];
            sum /= n;
            pbar[tid] = sum;
        }
    };
    // :278-295 per coordinate: the two probes and what the restore leaves behind
    auto probe_terms = [&] {
        if (tid < n) {
            const double del = step[tid] * c.eps;
            const double a = xm[tid] + del;
            const double b = a - (del + del);
            fa[tid] = a;
            fb[tid] = b;
            fd[tid] = b + del;
        }
    };
    // coordinate j of probe r: the drifted coordinates in front of its own, the untouched ones behind
    auto probe_at = [&](int r, int j) {
        const int i = r >> 1;
        return j < i ? fd[j] : j == i ? ((r & 1) ? fb[j] : fa[j]) : xm[j];
    };
    // the value of one point in LDS, by wavefront 0, into vals[0]
    auto eval_point = [&](const double *x) {
        __syncthreads();
        if (w == 0) {
            const double f = nm_value(c, x, d.aux, lane);
            if (lane == 0) vals[0] = f;
        }
    };
    // the values of the simplex's rows into vals, the wavefronts taking rows in turn
    auto eval_rows = [&] {
        __syncthreads();
        for (int j = w; j < n1; j += nw) {
            const double f = nm_value(c, S + (size_t) j * ld, d.aux, lane);
            if (lane == 0) vals[j] = f;
        }
    };
    // :203-225 behind the step's replacement of row ihi
    auto finish_step = [&](int branch) {
        __syncthreads();
        s.branch = branch;
        if (ys[s.ihi] < s.ylo) {
            s.ylo = ys[s.ihi];
            s.ilo = s.ihi;
        }
        s.jcount--;
        if (0 < s.jcount) {
            s.conv = 0;
        } else if (s.fev <= c.mfev) {
            s.jcount = c.checkev;
            double sum = 0.;
            for (int k = 0; k < n1; k++) sum += ys[k];
            sum = sum / (n + 1.);
            double sumsq = 0.;
            for (int k = 0; k < n1; k++) sumsq += (ys[k] - sum) * (ys[k] - sum);
            if (sumsq <= c.rq) s.conv = 1;
        }
        s.it++;
        s.stage = NM_IDLE;
    };
    // row ihi takes x with the value f
    auto replace = [&](const double *x, double f) {
        if (tid < n) S[(size_t) s.ihi * ld + tid] = x[tid];
        if (tid == 0) ys[s.ihi] = f;
    };
    auto first_min = [&] {
        int ilo = 0;
        double mn = ys[0];
        for (int k = 1; k < n1; k++)
            if (ys[k] < mn) {
                mn = ys[k];
                ilo = k;
            }
        s.ilo = ilo;
        s.ylo = mn;
    };

    if (absorb && (s.stage == NM_WAIT_REFLECT || s.stage == NM_WAIT_SECOND)) centroid();
    if (absorb && s.stage == NM_WAIT_FACT) probe_terms();

    for (;;) {
        __syncthreads();
        if (s.stage == NM_BUILD) {                      // :312-367
            const double *st = d.start + pv;
            if (tid < n) {
                const int j = tid;
                const double x = st[j], sd = step[j] * s.del;
                double diag = x, off = x;
                if (c.minit == 0) {
                    diag = x + sd;
                } else if (c.minit == 1) {
                    diag = x + sd * c.sp;
                    off = x + sd * c.sq;
                } else if (c.minit == 2) {
                    diag = x == 0. ? 0.0075 : x * (1. + 0.05);
                }
                S[(size_t) n * ld + j] = x;
                if (c.minit != 3) {
                    for (int i = 0; i < n; i++) S[(size_t) i * ld + j] = i == j ? diag : off;
                } else {
                    const double a = d.lower[j], b = d.upper[j];
                    const double lo = a < b ? a : b, hi = a < b ? b : a;
                    for (int i = 0; i < n; i++) {
                        const u32x4 r = philox4x32_10(c.seed, (uint32_t) s.restarts, (uint32_t) i, (uint32_t) j,
                                stream_word(STREAM_NM_INIT, (uint32_t) (c.substream + p)));
                        S[(size_t) i * ld + j] = u01(r.x, r.y) * (hi - lo) + lo;
                    }
                }
            }
            s.stage = NM_WAIT_INIT;
            if (mode != NM_FUSED) {
                s.pending = n1;
                break;
            }
            eval_rows();
            continue;
        }
        if (s.stage == NM_WAIT_INIT || s.stage == NM_WAIT_SHRINK) {     // :252-260, :168-173
            for (int q = tid; q < n1; q += nt) ys[q] = vals[q];
            __syncthreads();
            s.fev += n1;
            first_min();
            s.conv = 0;
            if (s.stage == NM_WAIT_SHRINK) s.it++;
            s.stage = NM_IDLE;
            continue;
        }
        if (s.stage == NM_IDLE) {
            if (c.honor_stop && (s.conv || s.fev >= c.mfev)) {          // :270-295
                if (tid < n) {
                    xm[tid] = S[(size_t) s.ilo * ld + tid];
                    d.xmin[pv + tid] = xm[tid];
                }
                s.ynl = ys[s.ilo];
                if (c.mfev < s.fev) {
                    s.stop = 2;
                    break;
                }
                probe_terms();
                __syncthreads();
                s.stage = NM_WAIT_FACT;
                if (mode != NM_FUSED) {
                    for (int r = w; r < 2 * n; r += nw)
                        for (int j = lane; j < n; j += 64) cand[(size_t) r * ld + j] = probe_at(r, j);
                    s.pending = 2 * n;
                    break;
                }
                // (every probe is evaluated; the count below takes them up to the first that improved)
                double *buf = w == 0 ? pstar : p2star;
                for (int r = w; r < 2 * n; r += nw) {
                    for (int j = lane; j < n; j += 64) buf[j] = probe_at(r, j);
                    wave_sync();
                    const double f = nm_value(c, buf, d.aux, lane);
                    if (lane == 0) vals[r] = f;
                    wave_sync();
                }
                continue;
            }
            if (s.it >= s.goal) break;
            {                                                           // :92-114
                int ihi = 0;
                double mx = ys[0];
                for (int k = 1; k < n1; k++)
                    if (mx < ys[k]) {
                        mx = ys[k];
                        ihi = k;
                    }
                s.ihi = ihi;
                s.ynl = mx;
                s.conv = 0;
            }
            centroid();
            if (tid < n) pstar[tid] = pbar[tid] + c.rcoef * (pbar[tid] - S[(size_t) s.ihi * ld + tid]);
            s.stage = NM_WAIT_REFLECT;
            if (mode != NM_FUSED) {
                if (tid < n) cand[tid] = pstar[tid];
                s.pending = 1;
                break;
            }
            eval_point(pstar);
            continue;
        }
        if (s.stage == NM_WAIT_REFLECT) {
            const double ystar = vals[0];
            s.ystar = ystar;
            s.fev++;
            if (ystar < s.ylo) {                                        // :117-125
                if (tid < n) p2star[tid] = pbar[tid] + c.ecoef * (pstar[tid] - pbar[tid]);
                s.kind = NM_EXPAND;
            } else {
                int l = 0;                                              // :138-143
                for (int k = 0; k < n1; k++)
                    if (ystar < ys[k]) l++;
                if (1 < l) {                                            // :144-148
                    __syncthreads();
                    replace(pstar, ystar);
                    finish_step(NM_BR_REFLECTED);
                    continue;
                }
                if (l == 0) {                                           // :151-155
                    if (tid < n) p2star[tid] = pbar[tid] + c.ccoef * (S[(size_t) s.ihi * ld + tid] - pbar[tid]);
                    s.kind = NM_INSIDE;
                } else {                                                // :184-187
                    if (tid < n) p2star[tid] = pbar[tid] + c.ccoef * (pstar[tid] - pbar[tid]);
                    s.kind = NM_OUTSIDE;
                }
            }
            s.stage = NM_WAIT_SECOND;
            if (mode != NM_FUSED) {
                if (tid < n) cand[ld + tid] = p2star[tid];
                s.pending = 1;
                break;
            }
            eval_point(p2star);
            continue;
        }
        if (s.stage == NM_WAIT_SECOND) {
            const double y2star = vals[0], ystar = s.ystar;
            s.fev++;
            __syncthreads();
            if (s.kind == NM_EXPAND) {                                  // :128-134
                if (ystar < y2star) {
                    replace(pstar, ystar);
                    finish_step(NM_BR_EXPAND_REFUSED);
                } else {
                    replace(p2star, y2star);
                    finish_step(NM_BR_EXPANDED);
                }
            } else if (s.kind == NM_INSIDE) {
                if (ys[s.ihi] < y2star) {                               // :160-167
                    if (tid < n)
                        for (int j = 0; j < n1; j++)
                            S[(size_t) j * ld + tid] = c.scoef * (S[(size_t) j * ld + tid] + S[(size_t) s.ilo * ld + tid]);
                    s.branch = NM_BR_SHRINK;
                    s.stage = NM_WAIT_SHRINK;
                    if (mode != NM_FUSED) {
                        s.pending = n1;
                        break;
                    }
                    eval_rows();
                } else {                                                // :178-179
                    replace(p2star, y2star);
                    finish_step(NM_BR_INSIDE);
                }
            } else if (y2star <= ystar) {                               // :192-194
                replace(p2star, y2star);
                finish_step(NM_BR_OUTSIDE);
            } else {                                                    // :196-197: pstar with the value y2star
                replace(pstar, c.repair ? ystar : y2star);
                finish_step(NM_BR_OUTSIDE_REFUSED);
            }
            continue;
        }
        // NM_WAIT_FACT: :283-302
        int hit = -1;
        for (int r = 0; r < 2 * n; r++)
            if (vals[r] < s.ynl) {
                hit = r;
                break;
            }
        s.stage = NM_IDLE;
        if (hit < 0) {
            s.fev += 2 * n;
            if (tid < n) d.xmin[pv + tid] = fd[tid];
            s.del = step[n - 1] * c.eps;
            s.stop = 1;
            break;
        }
        s.fev += hit + 1;
        if (tid < n) {
            const double v = probe_at(hit, tid);
            d.xmin[pv + tid] = v;
            d.start[pv + tid] = v;
        }
        s.del = c.eps;
        s.restarts++;
        s.conv = 0;
        s.stage = NM_BUILD;
    }

    __syncthreads();
    if (c.lds)
        for (int q = tid; q < n1 * ld; q += nt) G[q] = S[q];
    for (int q = tid; q < n1; q += nt) d.y[(size_t) p * n1 + q] = ys[q];
    if (tid == 0) d.scal[p] = s;
}
#endif

// A fresh start of population p at `from` (n doubles), by the workgroup that calls it: exactly the state init()
// uploads -- start, xmin zero, the fresh scalars (del = 1 on step = rad0, stage NM_BUILD, jcount = checkev, the
// counters and stop zero).  The simplex, y, cand and value are written by the walk before it reads them.  The
// next launch of nm_walk under honor_stop builds the simplex and goes on as nelmin() does (BasinHopping's hops).
__device__ inline void nm_rearm(const NmDev &d, const NmConst &c, int p, const double *from, int tid, int nt)
{
    const size_t pv = (size_t) p * c.ld;
    for (int j = tid; j < c.ld; j += nt) {
        d.start[pv + j] = j < c.n ? from[j] : 0.;
        d.xmin[pv + j] = 0.;
    }
    if (tid == 0) d.scal[p] = nm_fresh_scal(c.checkev);
}

// where the pending batch of a population lies: rows of the simplex, or rows of cand
__device__ inline const double *nm_pending_rows(const NmDev &d, const NmConst &c, int p, int stage)
{
    if (stage == NM_WAIT_INIT || stage == NM_WAIT_SHRINK) return d.P + (size_t) p * (c.n + 1) * c.ld;
    const double *cand = d.cand + (size_t) p * 2 * c.n * c.ld;
    return stage == NM_WAIT_SECOND ? cand + c.ld : cand;
}

#ifndef BBO_WALK_DEVICE_FUNCTIONS_ONLY
// the built-in at every population's pending batch (bbo_nm_phase 1).  grid (P), NM_THREADS threads
__global__ __launch_bounds__(NM_THREADS) void nm_eval(NmDev d, NmConst c)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const NmScal *sc = d.scal + p;
    if (!sc->pending || pop_frozen(c, sc)) return;
    const double *rows = nm_pending_rows(d, c, p, sc->stage);
    for (int r = w; r < sc->pending; r += NM_THREADS / 64) {
        const double f = nm_value(c, rows + (size_t) r * c.ld, d.aux, lane);
        if (lane == 0) d.value[(size_t) p * c.vs + r] = f;
    }
}
#endif

} // namespace bbo
