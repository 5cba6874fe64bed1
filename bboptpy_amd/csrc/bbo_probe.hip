// bbo_probe.hip -- diagnostics: one built-in objective through ONE of its device forms, at points the
// caller supplies (bbo_probe_objective in include/bbopt_hip.h).  The optimizers reach these forms only
// with the candidates they draw themselves; the probe feeds them the optimum, the octant seams of
// cos_2pi, huge and tiny arguments, and returns the raw value: no NaN guard, no ranking.
//
// The padding of every staged row holds POISON (1e300), not zero: a term that reads a column at or
// beyond n then shows in the value.  That includes the accumulator form: its callers zero the columns
// from n to 128, but eval_frag_rows masks every term by its column and must not depend on that (a
// poisoned neighbour makes Rosenbrock's masked term inf, which the select discards).
#include "bbo_common.hpp"
#include "bbo_objectives.hpp"

namespace bbo {

namespace {

constexpr double PROBE_POISON = 1.0e300;
constexpr int PROBE_MAX_N = 1024;       // 4 staged rows of round_up(n, 64) + 64 doubles stay under 64 KiB of LDS
constexpr int PROBE_FRAG_LD = 128;      // eval_frag_rows<8>: 8 column tiles of 16

__host__ __device__ inline int probe_lds_ld(int n) { return (n + 63) / 64 * 64 + 64; }

// forms 0..3: one wavefront per workgroup, 64 / G rows in it.  STAGE: the row is copied into LDS (at
// row_swizzle(j) when SWZ) over a row of poison; else it is read where it lies, row stride ld.
template<int G, bool SWZ, int UNR, bool STAGE>
__global__ __launch_bounds__(64) void probe_row_group(int obj, int n, int rows, int ld, const double *X,
        const double *aux, double *f_out)
{
    extern __shared__ double probe_stage[];
    const int grp = threadIdx.x / G, g = threadIdx.x % G;
    const int row = blockIdx.x * (64 / G) + grp;
    const bool live = row < rows;
    const double *xrow = X + (size_t) (live ? row : 0) * ld;
    if (STAGE) {
        const int sld = probe_lds_ld(n);
        double *mine = probe_stage + grp * sld;
        for (int j = g; j < sld; j += G) mine[j] = PROBE_POISON;
        __syncthreads();
        for (int j = g; j < n; j += G) mine[SWZ ? row_swizzle(j) : j] = xrow[j];
        __syncthreads();
        xrow = mine;
    }
    // (every lane of every group evaluates: the butterflies need their partners)
    const double f = eval_row_group<G, SWZ, UNR>(obj, n, xrow, aux, g);
    if (live && g == 0) f_out[row] = f;
}

// form 4: x[t][r] straight from memory in the accumulator layout -- column 16 t + (lane & 15) of row
// (lane >> 4) + 4 r -- 16 rows per wavefront, rows of PROBE_FRAG_LD doubles, poison behind n and in the
// rows that fill the last group of 16
__global__ __launch_bounds__(64) void probe_frag_rows(int obj, int n, int rows, const double *X,
        const double *aux, double *f_out)
{
    const int lane = threadIdx.x, c0 = lane & 15;
    double x[8][4], f[4];
#pragma unroll
    for (int t = 0; t < 8; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = blockIdx.x * 16 + (lane >> 4) + 4 * r;
            x[t][r] = X[(size_t) row * PROBE_FRAG_LD + 16 * t + c0];
        }
    eval_frag_rows<8>(obj, n, x, aux, lane, f);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = blockIdx.x * 16 + (lane >> 4) + 4 * r;
        if (c0 == 0 && row < rows) f_out[row] = f[r];
    }
}

template<int G, bool SWZ, int UNR, bool STAGE>
void launch_row_group(int obj, int n, int rows, int ld, const double *X, const double *aux, double *f)
{
    const int rpb = 64 / G;
    // (at most 4 rows of 1088 doubles: 34 KiB, under the default ceiling of dynamic LDS)
    const size_t lds = STAGE ? (size_t) rpb * probe_lds_ld(n) * sizeof(double) : 0;
    probe_row_group<G, SWZ, UNR, STAGE><<<(rows + rpb - 1) / rpb, 64, lds>>>(obj, n, rows, ld, X, aux, f);
}

} // namespace

void probe_objective(int obj, int form, int n, int rows, const double *X, double *f_out)
{
    BBO_REQUIRE(X && f_out, "bbo_probe_objective: NULL argument");
    BBO_REQUIRE(obj >= 0 && obj < OBJ_COUNT, "bbo_probe_objective: unknown objective");
    BBO_REQUIRE(form >= 0 && form <= 4, "bbo_probe_objective: form must be 0..4");
    BBO_REQUIRE(rows >= 1 && rows <= 65536, "bbo_probe_objective: rows must be in [1, 65536]");
    BBO_REQUIRE(n >= 1 && n <= PROBE_MAX_N, "bbo_probe_objective: n must be in [1, 1024]");
    if (form == 4) {
        BBO_REQUIRE(n <= PROBE_FRAG_LD, "bbo_probe_objective: the accumulator form takes n <= 128");
        BBO_REQUIRE(frag_objective_ok(obj),
                "bbo_probe_objective: the accumulator form does not offer this objective");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        throw Error(BBO_ERR_NO_DEVICE, "bbo_probe_objective: no HIP device");

    // the rows as the form reads them: ld = n for the staged forms (the kernel pads in LDS),
    // round_up(n, 2) for the global form, 128 and whole groups of 16 rows for the accumulator form;
    // behind the last row two more poisoned doubles, so that a read past it shows instead of faulting
    const int ld = form == 4 ? PROBE_FRAG_LD : form == 1 ? round_up(n, 2) : n;
    const int rows_staged = form == 4 ? round_up(rows, 16) : rows;
    std::vector<double> hx((size_t) rows_staged * ld + 2, PROBE_POISON);
    for (int r = 0; r < rows; r++) std::memcpy(&hx[(size_t) r * ld], X + (size_t) r * n, n * sizeof(double));
    // the table, poisoned behind n as well (at least 128 entries: the accumulator form indexes up to 127)
    std::vector<double> haux((size_t) (n > PROBE_FRAG_LD ? n : PROBE_FRAG_LD) + 64, PROBE_POISON);
    fill_objective_aux(obj, n, haux.data());

    DevBuf<double> dx, daux, df;
    dx.alloc(hx.size());
    daux.alloc(haux.size());
    df.alloc(rows);
    dx.upload(hx.data(), hx.size());
    daux.upload(haux.data(), haux.size());
    switch (form) {
    case 0: launch_row_group<16, false, 1, true>(obj, n, rows, ld, dx.p, daux.p, df.p); break;
    case 1: launch_row_group<64, false, 1, false>(obj, n, rows, ld, dx.p, daux.p, df.p); break;
    case 2: launch_row_group<64, true, 1, true>(obj, n, rows, ld, dx.p, daux.p, df.p); break;
    case 3: launch_row_group<16, false, 4, true>(obj, n, rows, ld, dx.p, daux.p, df.p); break;
    default: probe_frag_rows<<<rows_staged / 16, 64>>>(obj, n, rows, dx.p, daux.p, df.p); break;
    }
    BBO_HIP(hipGetLastError());
    BBO_HIP(hipDeviceSynchronize());
    df.download(f_out, rows);
}

} // namespace bbo
