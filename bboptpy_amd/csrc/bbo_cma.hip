// bbo_cma.hip -- host side of the CMA-ES / active CMA-ES engine: strategy constants,
// HBM state, and the kernel sequence of one generation.
//
// Reference behaviour restated on the host: BaseCmaes::init (base_cmaes.cpp:54-134),
// Cmaes::init (cmaes.cpp:44-63), ActiveCmaes::init (active_cmaes.cpp:42-69),
// CholeskyCmaes::init (cholesky_cmaes.cpp:40-52),
// BaseCmaes::setParams (:136-148), optimize (:162-174), solution (:158-160).
#include "bbo_cma_kernels.hpp"
#include "bbo_sep_kernels.hpp"
#include "bbo_chol_kernels.hpp"
#include "bbo_eig_mw.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <limits>

namespace bbo {

namespace {

// kernel slots of the profile report (bbo_get "profile"), in launch order
enum { K_SAMPLE = 0, K_RANK, K_WHITEN, K_GRAM, K_PATHS, K_COV, K_EIGEN, K_POST, K_STOP, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:cma_sample_eval", "bbo:cma_rank", "bbo:cma_whiten", "bbo:cma_gram", "bbo:cma_paths", "bbo:cma_cov", "bbo:cma_eigen", "bbo:cma_post", "bbo:cma_history_stop" };   // roctx ranges, bench.py's slot names

int pick_maxt(int ld)
{
    const int per_wave = ((ld >> 4) + 3) / 4;
    if (per_wave <= 1) return 1;
    if (per_wave <= 2) return 2;
    if (per_wave <= 4) return 4;
    return 8;
}

// rows a workgroup of the n = 128 batch kernels walks: one workgroup per CU when the rows in flight allow
// it (long tile loops amortise the fill of the operand), in steps of 128, at most `cap`
int rows_per_workgroup(long rows, int cap)
{
    const int rw = (int) ((rows / 256 + 127) / 128) * 128;
    return std::max(128, std::min(cap, rw));
}

// sep_sample_sum is built per objective: the instantiation of obj (sep_sum_objective holds)
template<int NC>
auto sep_sum_kernel(int obj) -> void (*)(CmaDev, CmaConst)
{
    switch (obj) {
    case OBJ_SPHERE: return sep_sample_sum<256, NC, OBJ_SPHERE>;
    case OBJ_ELLIPSOID: return sep_sample_sum<256, NC, OBJ_ELLIPSOID>;
    case OBJ_RASTRIGIN: return sep_sample_sum<256, NC, OBJ_RASTRIGIN>;
    case OBJ_CIGAR: return sep_sample_sum<256, NC, OBJ_CIGAR>;
    case OBJ_DISCUS: return sep_sample_sum<256, NC, OBJ_DISCUS>;
    default: return sep_sample_sum<256, NC, OBJ_DIFFPOW>;
    }
}

int gram_ldy(int ld)
{
    // rows k, k+1 of the slab must land 32 banks apart for the k-major fragment reads
    return (ld % 32 == 0) ? ld + 16 : ld;
}

// dynamic LDS of cma_gram: the slab, its two coefficient columns, the mean's partial sums
constexpr size_t GRAM_LDS_MAX = 160 * 1024 - 64;
size_t gram_lds_bytes(int ld, int rps)
{
    const int rpp = 256 / (ld / 4) > 0 ? 256 / (ld / 4) : 1;
    return ((size_t) rps * gram_ldy(ld) + 2 * (size_t) rps + (size_t) rpp * ld) * sizeof(double);
}

// where element (i, j) of an ld x ld matrix sits in MFMA B-fragment order (BDp, ISp; the kernels'
// packed operands): tile i >> 4, k-step j >> 2 of ld / 4, lane (j & 3, i & 15) of 64
inline size_t bfrag_index(size_t i, size_t j, size_t ld)
{
    return ((i >> 4) * (ld >> 2) + (j >> 2)) * 64 + ((j & 3) << 4) + (i & 15);
}

} // namespace

CmaEngine::CmaEngine(const bbo_params &p) :
        Engine(checked(p))
{
    BBO_HIP(hipHostMalloc((void**) &mw_fail_host_, sizeof(int)));
    *mw_fail_host_ = 0;
}

// the algorithm's own parameter checks, ahead of the base's (populations, device)
const bbo_params &CmaEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_CMAES || p.algo == BBO_ALGO_ACTIVE_CMAES
            || p.algo == BBO_ALGO_SEP_CMAES || p.algo == BBO_ALGO_CHOLESKY_CMAES,
            "CmaEngine: algo must be CMAES, ACTIVE_CMAES, SEP_CMAES or CHOLESKY_CMAES");
    BBO_REQUIRE(p.np >= 4, "CMA-ES needs np >= 4 (mu >= 2, best/worst pairs)");
    return p;
}

CmaEngine::~CmaEngine()
{
    mw_release();
    if (mw_fail_host_) (void) hipHostFree(mw_fail_host_);
}

// ---- the spread reduction's share of the device (bbo_eig_mw.hpp) -----------------------------------
// Its workgroups wait for each other, so all of them -- of every engine of this process that may
// have such a kernel in flight on the device -- must be resident at once.  Capacity: compute units
// (hipDeviceProp) x workgroups of cma_tred_mw512 a compute unit holds (the occupancy API; 1 on
// gfx950: 277 / 512 registers per lane), minus a margin of a sixteenth for whatever else runs.  An
// engine reserves its count before its first spread launch and gives it back when it dies, changes
// shape or falls back; who gets no reservation uses the one-workgroup reduction.  Other PROCESSES
// on the device are not seen: against them stands the bounded wait and the fallback.
namespace {
struct MwBudget {
    static constexpr int MAXDEV = 64;
    std::mutex m;
    long cap[MAXDEV] = {};
    long used[MAXDEV] = {};
    bool known[MAXDEV] = {};
    static MwBudget &get()
    {
        // (never destroyed: an engine that outlives the library's static objects -- a global in the
        // caller's program -- still gives its share back through a live object)
        static MwBudget *b = new MwBudget;
        return *b;
    }
    long capacity(int dev)
    {
        if (!known[dev]) {
            hipDeviceProp_t prop;
            int per_cu = 0;
            long cus = 0;
            if (hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*) cma_tred_mw512, MW_T, 0)
                    != hipSuccess || per_cu < 1)
                per_cu = 1;
            cap[dev] = cus * per_cu - std::max(1L, cus / 16);
            known[dev] = true;
        }
        return cap[dev];
    }
    bool reserve(int dev, long wgs)
    {
        if (dev < 0 || dev >= MAXDEV) return false;
        std::lock_guard<std::mutex> lock(m);
        if (used[dev] + wgs > capacity(dev)) return false;
        used[dev] += wgs;
        return true;
    }
    void release(int dev, long wgs)
    {
        if (dev < 0 || dev >= MAXDEV) return;
        std::lock_guard<std::mutex> lock(m);
        used[dev] -= wgs;
    }
};
} // namespace

// fault injection for the tests of the spread reduction: the ENVIRONMENT of this process only
// (read when an engine is initialised and on the phase-by-phase path the tests drive; bbo_set
// cannot reach it)
static int mw_fault_from_env()
{
    const char *e = std::getenv("BBO_MW_FAULT_STEP");
    return e && *e ? std::atoi(e) : -1;
}

bool CmaEngine::mw_reserve(long workgroups)
{
    if (mw_reserved_ == workgroups) return true;
    mw_release();
    if (!MwBudget::get().reserve(params_.device, workgroups)) return false;
    mw_reserved_ = workgroups;
    return true;
}

void CmaEngine::mw_release()
{
    if (mw_reserved_ > 0) MwBudget::get().release(params_.device, mw_reserved_);
    mw_reserved_ = 0;
}

// after a synchronisation of the stream: did a spread reduction launched since the last look give up?
bool CmaEngine::mw_check_failed()
{
    if (!mw_launched_) return false;
    mw_launched_ = false;
    if (!*mw_fail_host_) return false;
    *mw_fail_host_ = 0;
    mw_disabled_ = true;
    mw_release();
    return true;
}

void CmaEngine::set_params(int np, double sigma, int mfev)
{
    params_.np = np;
    params_.sigma0 = sigma;
    params_.mfev = mfev;
    if (params_.bound) {
        params_.bound = 0;
        fprintf(stderr, "Warning [CMA]: box bounding is no longer enabled.\n");
    }
}

void CmaEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    const bool chol = params_.algo == BBO_ALGO_CHOLESKY_CMAES;
    const bool sep = params_.algo == BBO_ALGO_SEP_CMAES;
    // dense: the variants with the eigen-state B, C, D, C^-1/2 (the Cholesky variant keeps its
    // factor A and the scratch image of C' instead, the separable one a diagonal)
    const bool dense = !sep && !chol;
    if (sep)
        BBO_REQUIRE(n >= 1 && n <= 4096, "SepCMAES: dimension must be in [1, 4096]");
    else
        BBO_REQUIRE(n >= 1 && n <= EIG_NMAX, "dimension must be in [1, 512]");
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations;
    const int lambda = params_.np;
    CmaConst &c = c_;
    c = CmaConst {};
    c.n = n;
    c.ld = round_up(n, 16);
    c.lambda = lambda;
    c.lambda_pad = round_up(lambda, 16);
    c.mu = lambda / 2;
    c.mu_pad = round_up(c.mu, 16);
    c.variant = chol ? 3 : sep ? 2 : params_.algo == BBO_ALGO_ACTIVE_CMAES ? 1 : 0;
    c.stol = params_.stol;
    c.ranked = params_.ranked ? 1 : 0;
    c.bound = params_.bound ? 1 : 0;
    // (16 < ld <= 128: the samplers there always hand down ||z||^2, so without a box nothing in
    // a generation reads C^-1/2 but cma_paths, which can work from B and D)
    c.lazy_isc = (dense && !c.bound && c.ld > 16 && c.ld <= 256) ? 1 : 0;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.mit = params_.mfev / lambda;
    c.npop = P;
    c.seed = params_.seed;
    c.tol = params_.tol;
    c.sigma0 = params_.sigma0;
    c.stop_off = 0;
    c.ftarget = -std::numeric_limits<double>::infinity();

    // recombination weights, base_cmaes.cpp:92-105
    std::vector<double> w(c.mu);
    double sum = 0.;
    for (int i = 0; i < c.mu; i++) {
        w[i] = std::log(0.5 * (lambda + 1.)) - std::log(i + 1.);
        sum += w[i];
    }
    const double inv = 1. / sum;
    for (int i = 0; i < c.mu; i++) w[i] *= inv;
    double lenw = 0.;
    for (int i = 0; i < c.mu; i++) lenw = lenw + w[i] * w[i];
    c.mueff = 1. / lenw;

    // base_cmaes.cpp:108-117
    c.chi = std::sqrt(n) * (1. - 1. / (4. * n) + 1. / (21. * n * n));
    c.cc = (4. + c.mueff / n) / (n + 4. + 2. * c.mueff / n);
    c.cs = (c.mueff + 2.) / (5. + n + c.mueff);
    c.c1 = 2. / ((1.3 + n) * (1.3 + n) + c.mueff);
    c.cmu = std::min(1. - c.c1,
            2. * (c.mueff - 2. + 1. / c.mueff) / ((2. + n) * (2. + n) + c.mueff));
    c.damps = 1. + c.cs + 2. * std::max(0., std::sqrt((c.mueff - 1.) / (n + 1.)) - 1.);
    c.hlen = 10 + (int) std::ceil((30. * n) / lambda);
    c.ik = (int) std::ceil(0.1 + lambda / 4.);
    // cmaes.cpp:48
    c.eigenfreq = params_.eigenrate * lambda / (c.c1 + c.cmu) / n;
    c.cm = 1.;
    c.alphaold = 0.5;
    c.cneg = 0.;
    if (c.variant == 1) {
        // active_cmaes.cpp:48-64
        const double ac = params_.alphacov;
        c.cc = (4. + 0. * c.mueff / n) / (n + 4. + 0. * 2. * c.mueff / n);
        c.cs = (c.mueff + 2.) / (3. + n + c.mueff);
        c.c1 = ac * std::min(1., lambda / 6.) / ((n + 1.3) * (n + 1.3) + c.mueff);
        c.cmu = 1. - c.c1;
        c.cmu = std::min(c.cmu,
                ac * (c.mueff - 2. + 1. / c.mueff) / ((2. + n) * (2. + n) + ac * c.mueff / 2.));
        c.cneg = (1. - c.cmu) * (ac / 8.) * c.mueff / (std::pow(n + 2., 1.5) + 2. * c.mueff);
        c.damps = 1. + c.cs + 2. * std::max(0., std::sqrt((c.mueff - 1.) / (n + 1.)) - 1.);
        c.eigenfreq = params_.eigenrate * (1. / (c.c1 + c.cmu + c.cneg)) / n;
    }

    if (sep) {
        // sep_cmaes.cpp:46-62
        c.cc = 4. / (n + 4.);
        c.cs = (c.mueff + 2.) / (3. + n + c.mueff);
        c.damps = 1. + c.cs + 2. * std::max(0., std::sqrt((c.mueff - 1.) / (n + 1.)) - 1.);
        c.ccov = 2. / ((n + std::sqrt(2.)) * (n + std::sqrt(2.)) * c.mueff);
        c.ccov += std::min(1., (2. * c.mueff - 1.) / ((n + 2.) * (n + 2.) + c.mueff))
                * (1. - 1. / c.mueff);
        if (params_.adjustlr) c.ccov *= ((n + 2.) / 3.);
    }

    // Gram split-K geometry: cma_gram holds its slab (rps rows of ldy doubles) in LDS
    c.rps = 64;
    while (c.rps > 16 && gram_lds_bytes(c.ld, c.rps) > GRAM_LDS_MAX) c.rps >>= 1;
    if (c.ld == 128) {
        // cma_gram128 streams its slab: size the slabs for ~512 workgroups over all populations
        // (two resident per CU: one round; 1024 cost 1 % more in the Gram kernel and a quarter more
        // in cma_cov, which sums the slabs)
        int cap = 32;
        if (const char *e = std::getenv("BBO_GRAM_WANT")) cap = std::max(1, std::atoi(e));     // (tuning)
        int want = std::max(1, std::min(cap, (512 + P - 1) / P));
        want = std::min(want, (c.lambda_pad + G128_CH - 1) / G128_CH);
        c.rps = ((c.lambda_pad + want - 1) / want + G128_CH - 1) / G128_CH * G128_CH;
    }
    c.splits = (c.lambda_pad + c.rps - 1) / c.rps;
    if (chol) c.splits = 1;      // (chol_cprime sums its rows inside one workgroup per tile)
    else if (sep)   // slabs of the mu selected ranks: enough workgroups to stream at HBM rate
        c.splits = std::max(1, std::min(c.mu / 16, (1024 + P - 1) / P));

    // ---- HBM state ------------------------------------------------------------
    const size_t ld = c.ld, ld2 = ld * ld;
    const bool same_shape = dense && keep_bc_ && last_n_ == n && C_.count == P * ld2;
    X_.alloc((size_t) P * c.lambda_pad * ld);
    f_.alloc((size_t) P * c.lambda_pad);
    zn2_.alloc((size_t) P * c.lambda_pad);
    rank_.alloc((size_t) P * c.lambda_pad);
    order_.alloc((size_t) P * c.lambda_pad);
    xmean_.alloc(P * ld);
    xold_.alloc(P * ld);
    pc_.alloc(P * ld);
    ps_.alloc(P * ld);
    D_.alloc(P * ld);
    csep_.alloc(P * ld);
    if (dense) {
        isc_.alloc(P * ld2);
        BDp_.alloc(P * ld2);
        ISp_.alloc(P * ld2);
    }
    if (chol) {
        // A = I (cholesky_cmaes.cpp:45-51: cleared at every init, nothing survives a re-init)
        A_.alloc(P * ld2);
        C_.alloc(P * ld2);
        BDp_.alloc(P * ld2);
        std::vector<double> eyeA(P * ld2, 0.), eyeP(P * ld2, 0.);
        for (int p = 0; p < P; p++)
            for (size_t i = 0; i < (size_t) n; i++) {
                eyeA[p * ld2 + i * ld + i] = 1.;
                eyeP[p * ld2 + bfrag_index(i, i, ld)] = 1.;
            }
        A_.upload(eyeA.data(), P * ld2);
        allow_lds((const void*) chol_factor, 136 * 1024);      // (ld <= 128: the matrix in LDS)
        std::vector<int> zero(P, 0);
        chol_repairs_.alloc(P);
        chol_repairs_.upload(zero.data(), P);
        BDp_.upload(eyeP.data(), P * ld2);
    }
    S_.alloc((size_t) P * c.mu_pad);
    // cma_gram128s' per-row coefficients, where cma_rank_sort can write them (zeroed: no stamp is valid)
    const bool coef_table = dense && c.ld == 128;
    coef_tab_.alloc(coef_table ? (size_t) P * coef_tab_chunks(c.lambda_pad) * 2 * G128_CH : 0);
    coef_stamp_.alloc(coef_table ? P : 0);
    gram_part_.alloc((size_t) P * c.splits * (dense ? ld2 : ld));   // sep: second moments, [ld]; Cholesky: unused
    mean_part_.alloc((size_t) P * c.splits * ld);
    hist_best_.alloc((size_t) P * c.hlen);
    hist_kth_.alloc((size_t) P * c.hlen);
    weights_.alloc(c.mu);
    weights_.upload(w.data(), c.mu);
    scal_.alloc(P);
    zinject_.release();
    zrecord_.release();
    upload_box(n, c.ld, lower, upper, obj);

    // B = C = C^-1/2 = I, D = 1.  The reference resize()s _b/_c, so on a re-init of the
    // SAME object with the same n the old off-diagonals survive and only the diagonals are
    // reset (cmaes.cpp:53-59); restart drivers depend on that, so it is kept.
    std::vector<double> eye(dense ? P * ld2 : 0, 0.), ones(P * ld, 1.);
    csep_.upload(ones.data(), P * ld);
    if (dense) {
        for (int p = 0; p < P; p++)
            for (int i = 0; i < n; i++) eye[p * ld2 + (size_t) i * ld + i] = 1.;
        if (same_shape) {
            std::vector<double> bm(P * ld2), cm(P * ld2);
            B_.download(bm.data(), P * ld2);
            C_.download(cm.data(), P * ld2);
            for (int p = 0; p < P; p++)
                for (int i = 0; i < n; i++) {
                    bm[p * ld2 + (size_t) i * ld + i] = 1.;
                    cm[p * ld2 + (size_t) i * ld + i] = 1.;
                }
            B_.upload(bm.data(), P * ld2);
            C_.upload(cm.data(), P * ld2);
        } else {
            B_.alloc(P * ld2);
            C_.alloc(P * ld2);
            B_.upload(eye.data(), P * ld2);
            C_.upload(eye.data(), P * ld2);
        }
        isc_.upload(eye.data(), P * ld2);
    }
    D_.upload(ones.data(), P * ld);
    keep_bc_ = dense;
    last_n_ = n;

    std::vector<double> xm(P * ld, 0.);
    for (int p = 0; p < P; p++) std::copy(guess + (size_t) p * n, guess + (size_t) (p + 1) * n,
            xm.begin() + p * ld);
    xmean_.upload(xm.data(), P * ld);

    std::vector<CmaScal> sc(P);
    for (auto &s : sc) {
        std::memset(&s, 0, sizeof(s));
        s.sigma = params_.sigma0;
        s.fbest = -std::numeric_limits<double>::infinity();
        s.fworst = std::numeric_limits<double>::infinity();
        s.hist_head = -1;
        // a re-initialised object keeps the off-diagonals of B (cmaes.cpp:53-59) while C^-1/2
        // restarts from I: the two disagree until the first decomposition
        s.basis_ok = same_shape ? 0 : 1;
    }
    scal_.upload(sc.data(), P);
    basis_maybe_stale_ = same_shape;

    // the eigensolver keeps its matrix in LDS when it fits
    // global scratch of the eigensolver: the work matrix when it does not fit LDS, or
    // (divide and conquer) the Householder matrix and the merge factor
    if (dense) eig_work_.alloc((size_t) P * 4 * eig_slab((int) ld));

    CmaDev &d = d_;
    d = CmaDev {};
    d.X = X_.p; d.f = f_.p; d.rank = rank_.p; d.order = order_.p;
    d.xmean = xmean_.p; d.xold = xold_.p; d.pc = pc_.p; d.ps = ps_.p;
    d.C = C_.p; d.B = B_.p; d.D = D_.p; d.isc = isc_.p; d.BDp = BDp_.p; d.ISp = ISp_.p;
    d.A = chol ? A_.p : nullptr;
    d.chol_repairs = chol ? chol_repairs_.p : nullptr;
    d.coef_tab = coef_tab_.p; d.coef_stamp = coef_stamp_.p;
    d.S = S_.p; d.zn2 = zn2_.p; d.csep = csep_.p; d.gram_part = gram_part_.p; d.mean_part = mean_part_.p;
    d.hist_best = hist_best_.p; d.hist_kth = hist_kth_.p; d.eig_work = eig_work_.p;
    d.weights = weights_.p; d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p;
    d.zinject = nullptr; d.zrecord = nullptr; d.scal = scal_.p;
    d.stamps = stamps_.p;
    d.mw_fail_host = mw_fail_host_;
    d.mw_fault = mw_fault_from_env();
    mw_release();          // (the shape may have changed: reserved again at the first spread launch)

    // an objective program: the plan is static (population p's candidates and fitness), a stopped
    // population is skipped by its flag; the padding rows' +inf is written once, here
    if (obj_.is_program()) {
        prog_.bind(obj_.program, params_.device, n, P);
        std::vector<ProgPlan> plan(P);
        for (int p = 0; p < P; p++)
            plan[p] = ProgPlan { X_.p + (size_t) p * c.lambda_pad * ld, f_.p + (size_t) p * c.lambda_pad, lambda,
                    c.ld };
        prog_.upload_plan(plan);
        std::vector<double> finf((size_t) P * c.lambda_pad, std::numeric_limits<double>::infinity());
        f_.upload(finf.data(), finf.size());
    } else
        prog_.unbind();

    // packed operands of the initial B, D, C^-1/2
    c.honor_stop = 0;
    inited_ = true;
    if (dense) {
        launch_post(2);
        BBO_HIP(hipGetLastError());
        BBO_HIP(hipStreamSynchronize(stream_));
    }
}

// ---- kernel launches ---------------------------------------------------------------
void CmaEngine::launch_post(int mode)
{
    const CmaConst &c = c_;
    if (c.ld <= 128) {
        const size_t lds = (size_t) (c.ld * (c.ld + 2) + c.ld) * sizeof(double);
        allow_lds((const void*) cma_post_mfma<1>, 140 * 1024);
        allow_lds((const void*) cma_post_mfma<4>, 140 * 1024);
        // few populations: four workgroups each (latency); many: one (no redundant staging)
        if (c.npop < 32)
            hipLaunchKernelGGL(cma_post_mfma<4>, dim3(c.npop, 4), dim3(256), lds, stream_, d_, c_,
                    mode);
        else
            hipLaunchKernelGGL(cma_post_mfma<1>, dim3(c.npop, 1), dim3(256), lds, stream_, d_, c_,
                    mode);
    } else {
        dim3 grid(c.ld / 16, c.ld / 16, c.npop);
        hipLaunchKernelGGL(cma_post, grid, dim3(256), 0, stream_, d_, c_, mode);
    }
}

// Which sampler serves this shape, objective and set of switches, and with what geometry: a decision from
// the engine's constants alone, like eig_route -- nothing is launched or allocated here.
SampleRoute CmaEngine::sample_route() const
{
    const CmaConst &c = c_;
    SampleRoute r {};
    r.gy = c.npop;
    r.writes_zn = c.variant != 2;
    auto is = [&r](SampleKernel k, int gx, int block, size_t lds) {
        r.k = k;
        r.gx = gx;
        r.block = block;
        r.lds = lds;
    };
    if (c.variant == 2) {
        // separable: 16 lanes per candidate for short rows, one wavefront per candidate beyond
        // (a workgroup stages the generator's table once and then walks chunks of candidates:
        // ~4096 workgroups in all, 16 per CU)
        const int per_pop = std::max(1, 4096 / c.npop);
        if (c.ld <= 256)     // (beyond that the 16-row LDS tile would leave one workgroup per CU)
            is(SK_SEP_16, std::min((c.lambda_pad + 15) / 16, per_pop), 256, (size_t) 16 * c.ld * sizeof(double));
        else if (c.ld <= 2048) {
            // 8 rows per workgroup of 512: rows + table leave room for two workgroups (16
            // wavefronts) per CU up to ld = 1024
            is(SK_SEP_64_512, std::min((c.lambda_pad + 7) / 8, per_pop), 512, (size_t) 8 * c.ld * sizeof(double));
            r.full = nothing_to_guard() ? 1 : 0;     // (the benchmark's SEP)
            if (r.full && sep_sum_objective(c.obj) && !(d_.dbg & DBG_SEP_ROWS_LDS))
                // sums of per-coordinate terms: no row in LDS (sep_sample_sum); 256-thread
                // workgroups, as many rows in flight as the registers allow.  NC = 4: the lane's 32
                // constants resident -- not for the cosine / pow objectives, which inline a long body per
                // coordinate: with them they spill or fall to one wavefront per SIMD (Rastrigin took 512
                // registers and ran slower than from LDS rows)
                is(c.ld == 1024 && c.obj != OBJ_RASTRIGIN && c.obj != OBJ_DIFFPOW ? SK_SEP_SUM4 : SK_SEP_SUM,
                        std::min(c.lambda_pad / (4 * SEP_K), per_pop), 256, 0);
            else if (r.full)
                r.k = SK_SEP_64_512_LEAN;
        } else
            is(SK_SEP_64, std::min((c.lambda_pad + 3) / 4, per_pop), 256, (size_t) 4 * c.ld * sizeof(double));
    } else if (c.ld == 128 && (long) c.npop * c.lambda_pad >= sample128_min_rows_
            && (c.obj < 0 || frag_objective_ok(c.obj))) {
        // whole populations in flight: packed operand in LDS, normals drawn into the A fragments
        // (CholeskyCMAES, lower-triangular operand: 36 of 64 block pairs)
        r.rows_per_wg = rows_per_workgroup((long) c.npop * c.lambda_pad, 4096);
        is(c.variant == 3 && chol_tri_ ? SK_EVAL128_TRI : SK_EVAL128, (c.lambda_pad + r.rows_per_wg - 1) / r.rows_per_wg,
                512, 128 * 1024);
        r.full = nothing_to_guard() ? 1 : 0;     // the lean build of the tile loop where nothing needs guarding (M, C3)
        // ... and its transposed form (coordinates along the accumulators, the objective in the lane) for the
        // objectives eval_frag_cols offers and for none on the device; Schwefel 1.2 scans across lanes: row layout
        r.transposed = r.full && !sample128_rowlayout_ && (c.obj < 0 || frag_cols_objective_ok(c.obj)) ? 1 : 0;
    } else if (c.ld == 128 && (long) c.npop * (c.lambda_pad / 16) <= sample_wide_max_tiles_)
        // one population at a time: a 16-row tile per WORKGROUP, one column tile per wavefront (the
        // form C5's handful of candidates takes at n = 256) -- a wavefront's chain is 32 MFMAs and
        // one Philox call instead of 256 and eight
        is(c.variant == 3 && chol_tri_ ? SK_TILE8_TRI : SK_TILE8, c.lambda_pad / 16, 512,
                (size_t) 16 * (c.ld + 2) * sizeof(double));
    else if (c.ld <= 128)
        // 64 candidates per workgroup, packed operand held in registers
        // (ld <= 32: 8 k-steps of operand in registers instead of 32: twice the occupancy)
        is(c.ld <= 32 ? SK_EVAL64_1_8 : c.ld <= 64 ? SK_EVAL64_1 : SK_EVAL64_2, (c.lambda_pad + 63) / 64, 256,
                (size_t) 64 * (c.ld + 2) * sizeof(double));
    else {
        const int tiles = c.lambda_pad / 16;
        const size_t lds = (size_t) 16 * (c.ld + 2) * sizeof(double);
        // a handful of row tiles on the whole chip (C5: two): one column tile per wavefront
        if ((long) tiles * c.npop <= 32 && c.ld <= 256 && !(d_.dbg & DBG_SAMPLE_4WAVES))
            is(SK_TILE16, tiles, 1024, lds);
        else       // (ld > 128: pick_maxt is 4 or 8)
            is(pick_maxt(c.ld) == 4 ? SK_EVAL_4 : SK_EVAL_8, tiles, 256, lds);
    }
    return r;
}

void CmaEngine::launch_sample_eval()
{
    const SampleRoute r = sample_route();
    auto go = [&](auto kernel, int allow, auto... args) {      // allow: the kernel's LDS attribute, 0 = the default
        if (allow) allow_lds((const void*) kernel, allow);
        hipLaunchKernelGGL(kernel, dim3(r.gx, r.gy), dim3(r.block), r.lds, stream_, d_, c_, args...);
    };
    timed(K_SAMPLE, [&] {
        switch (r.k) {
        case SK_NONE: break;
        case SK_SEP_16: go(sep_sample_eval<16>, 128 * 1024); break;
        case SK_SEP_64_512: go(sep_sample_eval<64, 512>, 140 * 1024); break;
        case SK_SEP_64_512_LEAN: go(sep_sample_eval<64, 512, true>, 140 * 1024); break;
        case SK_SEP_SUM: go(sep_sum_kernel<0>(c_.obj), 0); break;
        case SK_SEP_SUM4: go(sep_sum_kernel<4>(c_.obj), 0); break;
        case SK_SEP_64: go(sep_sample_eval<64>, 140 * 1024); break;
        case SK_EVAL128: go(cma_sample_eval128, 128 * 1024, r.rows_per_wg, r.full, r.transposed); break;
        case SK_EVAL128_TRI: go(cma_sample_eval128_tri, 128 * 1024, r.rows_per_wg, r.full, r.transposed); break;
        case SK_TILE8: go(cma_sample_eval<1, 8>, 0); break;
        case SK_TILE8_TRI: go(cma_sample_eval<1, 8, true>, 0); break;
        case SK_EVAL64_1_8: go(cma_sample_eval64<1, 8>, 0); break;
        case SK_EVAL64_1: go(cma_sample_eval64<1>, 80 * 1024); break;
        case SK_EVAL64_2: go(cma_sample_eval64<2>, 80 * 1024); break;
        case SK_TILE16: go(cma_sample_eval<1, 16>, 0); break;
        case SK_EVAL_4: go(cma_sample_eval<4>, 0); break;
        case SK_EVAL_8: go(cma_sample_eval<8>, 80 * 1024); break;      // ld = 512: 65 792 bytes
        }
    });
    // ||z||^2 stands in for the whitened norm only if this launch wrote it and no x was clamped
    c_.use_zn = (r.writes_zn && !c_.bound) ? 1 : 0;
    last_sample_ = r;
}

void CmaEngine::launch_rank()
{
    const CmaConst &c = c_;
    rank_wrote_norms_ = false;
    // (which form, and why: rank_route, bbo_rank.hpp)
    last_rank_ = rank_route(c.lambda, c.npop, d_.dbg);
    timed(K_RANK, [&] {
        switch (last_rank_) {
        case RK_WAVE:
            hipLaunchKernelGGL(cma_rank_wave, dim3((c.npop + 3) / 4), dim3(256), 0, stream_, d_, c_);
            break;
        case RK_COUNT64:
            hipLaunchKernelGGL(cma_rank64, dim3((c.lambda + 3) / 4, c.npop), dim3(256), 0, stream_, d_, c_);
            break;
        case RK_COUNT32:
            hipLaunchKernelGGL(cma_rank32, dim3((c.lambda + 7) / 8, c.npop), dim3(256), 0, stream_, d_, c_);
            break;
        case RK_COUNT8:
            hipLaunchKernelGGL(cma_rank, dim3((c.lambda + 31) / 32, c.npop), dim3(256), 0, stream_, d_, c_);
            break;
        default: {   // the in-LDS sorts: cma_rank_sort picks the instantiation from m and dbg like rank_route
            const int m = rank_sort_m(c.lambda);
            allow_lds((const void*) cma_rank_sort, 128 * 1024);
            const size_t lds = rank_sort_merges(m, d_.dbg) ? (size_t) m * 24 : (size_t) std::max(m, 1024) * 12;
            hipLaunchKernelGGL(cma_rank_sort, dim3(c.npop), dim3(sort_threads(m)), lds, stream_, d_,
                    c_, m);
            break;
        }
        }
    });
    // the whitened norms of the worst mu, where they are the sampler's sigma^2 ||z||^2 handed
    // round through the ranking (cma_whiten128's shortcut): written by the sort itself, which
    // has the ranking in LDS, and by cma_rank_body -- a launch less per generation (10 us of the
    // M step).  Not by the one-wavefront form.
    if (last_rank_ != RK_WAVE) rank_wrote_norms_ = c.variant == 1 && c.use_zn && !basis_maybe_stale_;
}

// The kernels of one update of the distribution, with their geometry: a decision like sample_route.
UpdateRoute CmaEngine::update_route(bool norms_done, bool with_cov) const
{
    const CmaConst &c = c_;
    UpdateRoute r {};
    auto add = [&r](UpdateKernel k, int slot, int gx, int gy, int gz, int block, size_t lds = 0, int arg = 0) {
        r.step[r.count++] = UpdateRoute::Step { k, slot, gx, gy, gz, block, lds, arg };
    };
    const int NT = c.ld / 16, LT = NT * (NT + 1) / 2;      // 16 x 16 tiles of a row, of the lower triangle
    if (c.variant == 3) {
        // paths and C' read the old factor; chol_factor (launch_eigen's slot in the order of a
        // generation, but part of this phase: BBO_PHASE_EIGEN does nothing here) writes the new one
        const int in_lds = c.ld <= 128 ? 1 : 0;
        add(UK_CHOL_PATHS, K_PATHS, c.npop, 1, 1, 256);
        add(UK_CHOL_CPRIME, K_GRAM, LT, c.npop, 1, 256);
        add(UK_CHOL_FACTOR, K_COV, c.npop, 1, 1, 256, in_lds ? (size_t) c.ld * (c.ld + 1) * sizeof(double) : 0, in_lds);
        return r;
    }
    if (c.variant == 2) {
        add(UK_SEP_MOMENTS, K_GRAM, c.splits, (c.ld + 511) / 512, c.npop, 256);
        add(UK_SEP_PATHS, K_PATHS, c.npop, 1, 1, 256);
        return r;
    }
    if (c.variant == 1 && !norms_done) {      // the whitened norms of the worst mu, where the ranking has not written them
        if (c.ld == 128 && (long) c.npop * c.mu_pad >= 256 * 128) {
            const int rw = rows_per_workgroup((long) c.npop * c.mu_pad, 2048);
            add(UK_WHITEN128, K_WHITEN, (c.mu_pad + rw - 1) / rw, c.npop, 1, 512, (size_t) (128 * 128 + 128) * sizeof(double),
                    rw);
        } else
            add(UK_WHITEN, K_WHITEN, c.mu_pad / 16, c.npop, 1, 256, (size_t) (16 * (c.ld + 2) + 64) * sizeof(double),
                    pick_maxt(c.ld));
    }
    if (c.ld != 128)
        add(UK_GRAM, K_GRAM, c.splits, (LT + 4 * GRAM_TPW - 1) / (4 * GRAM_TPW), c.npop, 256, gram_lds_bytes(c.ld, c.rps),
                gram_ldy(c.ld));
    else if (d_.dbg & DBG_GRAM128_LDS)      // (diagnostic: the LDS-staged form, same bits)
        add(UK_GRAM128, K_GRAM, c.splits, c.npop, 1, 256, (size_t) (2 * G128_CH * G128_LDY + 4 * G128_CH) * sizeof(double));
    else
        add(UK_GRAM128S, K_GRAM, c.splits, c.npop, 1, 256);
    if (c.lazy_isc && c.n >= 64 && !(d_.dbg & DBG_PATHS_LAZY256))
        // (1024 threads: a quarter of the dependent round trips of the two passes over B)
        add(UK_PATHS_LAZY1K, K_PATHS, c.npop, 1, 1, 1024);
    else
        add(c.lazy_isc ? UK_PATHS_LAZY : UK_PATHS, K_PATHS, c.npop, 1, 1, 256);
    // (with_cov == false: the fixed-shape eigensolver that follows forms C on its load, and the slot
    // is not opened -- a slot without calls is left out of the kernel table)
    if (with_cov) add(UK_COV, K_COV, (c.n * (c.n + 1) / 2 + 255) / 256, c.npop, 1, 256);
    return r;
}

// cma_whiten<MAXT> of pick_maxt's four values (the one place they are switched on: the samplers of ld > 128
// are two ids of SampleKernel)
static auto whiten_kernel(int maxt) -> void (*)(CmaDev, CmaConst)
{
    switch (maxt) {
    case 1: return cma_whiten<1>;
    case 2: return cma_whiten<2>;
    case 4: return cma_whiten<4>;
    default: return cma_whiten<8>;
    }
}

void CmaEngine::launch_update(bool with_cov)
{
    const bool norms_done = rank_wrote_norms_;
    rank_wrote_norms_ = false;             // (one ranking serves one update)
    const UpdateRoute r = update_route(norms_done, with_cov);
    for (int i = 0; i < r.count; i++) {
        const UpdateRoute::Step &s = r.step[i];
        auto go = [&](auto kernel, int allow, auto... args) {      // allow: the kernel's LDS attribute, 0 = the default
            if (allow) allow_lds((const void*) kernel, allow);
            hipLaunchKernelGGL(kernel, dim3(s.gx, s.gy, s.gz), dim3(s.block), s.lds, stream_, d_, c_, args...);
        };
        timed(s.slot, [&] {
            switch (s.k) {
            case UK_CHOL_PATHS: go(chol_paths, 0); break;
            case UK_CHOL_CPRIME: go(chol_cprime, 0); break;
            case UK_CHOL_FACTOR: go(chol_factor, 0, s.arg); break;
            case UK_SEP_MOMENTS: go(sep_moments, 0); break;
            case UK_SEP_PATHS: go(sep_paths, 0); break;
            case UK_WHITEN128: go(cma_whiten128, 132 * 1024, s.arg); break;
            case UK_WHITEN: go(whiten_kernel(s.arg), s.arg == 8 ? 80 * 1024 : 0); break;      // ld = 512: 66 304 bytes
            case UK_GRAM128S: go(cma_gram128s, 0); break;
            case UK_GRAM128: go(cma_gram128, 80 * 1024); break;
            case UK_GRAM: go(cma_gram, (int) GRAM_LDS_MAX, s.arg); break;
            case UK_PATHS: go(cma_paths, 0); break;
            case UK_PATHS_LAZY: go(cma_paths_lazy, 0); break;
            case UK_PATHS_LAZY1K: go(cma_paths_lazy1k, 0); break;
            case UK_COV: go(cma_cov, 0); break;
            }
        });
    }
    last_update_ = r;
}

int CmaEngine::next_mw_xcd()
{
    static std::atomic<int> counter { 0 };
    return counter.fetch_add(1) & 7;
}

// What one decomposition launches, from the engine's constants and switches alone: nothing is launched,
// allocated or reserved here.  launch_eigen walks the result; generation() asks first, because in front
// of a route that forms C it leaves cma_cov out -- one function, so the two cannot disagree.
EigRoute CmaEngine::eig_route(bool spread_ok, bool fuse_ok) const
{
    const CmaConst &c = c_;
    const int dbg = d_.dbg;
    EigRoute r {};
    if (c.variant >= 2) return r;      // diagonal covariance: d = sqrt(c) is part of sep_paths; Cholesky: no decomposition
    auto add = [&r](EigKernel k, int arg = 0) { r.step[r.count++] = EigRoute::Step { k, arg }; };
    // 64 < n <= 128 with few matrices in flight (one optimisation run at a time): split over kernels the
    // way 128 < n <= 256 is (DBG_EIG_ONE_WG: everything on the reducing workgroup, as for a batch)
    const EigPlan pl_lds = eig_plan(c.n, c.ld);
    r.split = pl_lds.use_lds && pl_lds.threads == 512 && pl_lds.dc && c.npop <= split_maxp_
            && !(dbg & (DBG_QL | DBG_DC_NO_MERGES | DBG_DC_NO_LEAVES | DBG_TRED_L2 | DBG_EIG_ONE_WG));
    const EigPlan pl = r.split ? eig_plan_split(c.n, c.ld) : pl_lds;
    spread_ok = spread_ok && !mw_disabled_;
    // the fixed-shape builds of n = ld = 128 (plan: EIG_FX_PLAN = eig_plan(128, 128)) read no switch and
    // write no clock: production settings only
    const bool fixed_shape = c.n == 128 && c.ld == 128 && !d_.stamps
            && !(dbg & (DBG_EIG_IN_KERNEL | DBG_EIG_GENERIC128));
    bool big_spread = false, wy4_packs = false, fcols_closed = false;
    if (c.n <= 16 && c.n >= 2 && c.ld == 16 && !(dbg & DBG_NO_EIGEN_SMALL))
        add(EK_EIGEN_SMALL);
    else if (pl.threads < 512)    // four lanes per row: smaller matrices, smaller workgroups, several per CU
        add(pl.threads == 128 ? EK_EIGEN_128 : EK_EIGEN_256);
    else if (fixed_shape && c.npop > split_maxp_ && c.lazy_isc) {
        // a batch: in a generation (DBG_COV_UNFUSED aside) the kernel forms C from the Gram slabs itself
        r.fixed = true;
        r.forms_c = fuse_ok && !(dbg & DBG_COV_UNFUSED);
        add(r.forms_c ? EK_EIGEN_FX128 : EK_EIGEN_FX128U);
    } else if (pl.use_lds)
        add(EK_EIGEN);
    else if (pl.hybrid && !(dbg & (DBG_QL | DBG_TRED_L2 | DBG_EIG_ONE_WG))) {
        // 128 < n <= 256 and the split form: reduction, the two halves side by side, top merge.  The
        // reduction of n > 128 is spread while all its workgroups can be resident at once next to those
        // of the process's other engines (they wait for each other: MwBudget above, bbo_eig_mw.hpp)
        if (r.split) {
            r.fixed = fixed_shape;
            add(r.fixed ? EK_EIGEN_R1_FX128 : EK_EIGEN_R1);
        } else if (spread_ok && !(dbg & DBG_TRED_ONE_WG)) {
            r.mw_workgroups = (long) c.npop * MW_G;
            const int istop = (dbg & DBG_TRED_ALL_SPREAD) ? 1 : 128;
            add(EK_TRED_MW, istop);
            if (istop > 1) add(EK_TRED_TAIL);
        } else
            add(EK_EIGEN_G1);
        add(EK_EIG_HALVES);
        // the top merge: with few matrices in flight the secular equation on workgroups of its own
        if ((long) c.npop * 8 <= 256 && !(dbg & DBG_TOP_ONE_KERNEL)) {
            add(EK_EIGEN_G2, 1);
            add(EK_EIG_SECULAR);
            // ... and behind it the Loewner vector and the columns of F, the closing repair / root with
            // them (even n: the T factors were built beside the halves)
            fcols_closed = !(c.n & 1) && c.lazy_isc && (long) c.npop * ((c.n + 15) / 16) <= 256
                    && !(dbg & (DBG_TOP_PART2 | DBG_WY_PER_WAVE));
            if (fcols_closed) {
                add(EK_EIG_LOWNER);
                add(EK_EIG_FCOLS);
            } else
                add(EK_EIGEN_G2, 2);
        } else
            add(EK_EIGEN_G2, 0);
    } else if (pl.hybrid)
        add(EK_EIGEN_G);          // (everything in one workgroup)
    else if (c.n > 256 && pl.dc && spread_ok && !(dbg & (DBG_QL | DBG_TRED_ONE_WG))) {
        // 256 < n <= 512, few matrices (while 16 workgroups per matrix fit the chip at once): the
        // structure of 128 < n <= 256 in front of the same divide and conquer; two spread kernels, down
        // to pivot row 256 and to 128 (DBG_TRED_ALL_SPREAD: the first one down to row 128)
        big_spread = true;
        r.mw_workgroups = (long) c.npop * 16;
        const bool chain = !(dbg & DBG_TRED_ALL_SPREAD);
        add(EK_TRED_MW512, chain ? 256 : 128);
        if (chain) add(EK_TRED_MW_CHAIN);
        add(EK_TRED_TAIL, chain ? 1 : 0);
        add(EK_EIGEN_B4);
    } else
        add(EK_EIGEN_B);
    r.timed = r.count;
    if (pl.dc && !pl.reg_path && (pl.hybrid || !(dbg & DBG_QL))) {
        // n > 128: the top merge's two products as whole-GPU kernels (few populations: 64 x 16 blocks)
        const long blocks = (c.n + 63) / 64;
        add(blocks * blocks * c.npop < 128 ? EK_EIG_GEMM1 : EK_EIG_GEMM, 0);
        if (big_spread)
            add(EK_EIG_WY4_512);
        else if ((dbg & DBG_QL) || !pl.hybrid)     // (n > 256, QL: Q_house was accumulated by the reduction)
            add(EK_EIG_GEMM, 1);
        else if ((long) c.npop * ((c.n + 15) / 16) <= 256 && !(dbg & DBG_WY_PER_WAVE)) {
            // (under lazy_isc the packed operand B D leaves with B: no cma_post launch)
            wy4_packs = c.lazy_isc != 0;
            add(EK_EIG_WY4, wy4_packs ? (fcols_closed ? 2 : 1) : 0);
        } else
            add(EK_EIG_WY);
    }
    // (lazy_isc: the eigensolver has written the packed B D itself and C^-1/2 is not formed)
    const bool packed_by_eigen = c.lazy_isc && pl.dc && pl.reg_path && !(dbg & DBG_QL);
    r.post = r.step[0].k != EK_EIGEN_SMALL && !packed_by_eigen && !wy4_packs;
    if (r.post) add(c.ld <= 128 ? EK_POST_MFMA : EK_POST);
    return r;
}

void CmaEngine::launch_eigen(EigRoute r)
{
    const CmaConst &c = c_;
    // (no reservation: the one-workgroup reduction; no spread route forms C, so fuse_ok as asked)
    if (r.mw_workgroups && !mw_reserve(r.mw_workgroups)) r = eig_route(false, r.forms_c);
    last_route_ = r;
    if (c.variant >= 2) return;
    const EigPlan pl_lds = eig_plan(c.n, c.ld), pl = r.split ? eig_plan_split(c.n, c.ld) : pl_lds;
    const EigFxArgs fa { d_.C, d_.B, d_.D, d_.BDp, d_.eig_work, d_.scal, c.eigenfreq, c.honor_stop,
            c.splits, c.variant, d_.gram_part, d_.pc, c.cc, c.c1, c.cmu, c.cneg, c.alphaold };
    auto per_matrix = [&](auto kernel, int threads, const EigPlan &p, auto... args) {   // one workgroup each
        allow_lds((const void*) kernel, 160 * 1024 - 768);
        hipLaunchKernelGGL(kernel, dim3(c.npop), dim3(threads), p.lds_bytes, stream_, args...);
    };
    auto per_columns = [&](auto kernel, int w, int threads, auto... args) {   // ceil(n / w) workgroups per matrix
        hipLaunchKernelGGL(kernel, dim3((c.n + w - 1) / w, c.npop), dim3(threads), 0, stream_, d_, c_, args...);
    };
    timer_.begin(stream_, K_EIGEN);     // (by hand: the slot closes at step r.timed, inside the loop)
    for (int i = 0; i < r.count; i++) {
        if (i == r.timed) {          // (the top merge's products are not part of the slot)
            timer_.end(stream_);
            BBO_HIP(hipGetLastError());
        }
        const int arg = r.step[i].arg;
        switch (r.step[i].k) {
        case EK_EIGEN_SMALL:
            hipLaunchKernelGGL(cma_eigen_small, dim3((c.npop + 3) / 4), dim3(256), 0, stream_, d_, c_, 0, 1);
            break;
        case EK_EIGEN_128: per_matrix(cma_eigen_128, 128, pl, d_, c_, pl, 0); break;
        case EK_EIGEN_256: per_matrix(cma_eigen_256, 256, pl, d_, c_, pl, 0); break;
        case EK_EIGEN: per_matrix(cma_eigen, 512, pl, d_, c_, pl, 0); break;
        case EK_EIGEN_FX128: per_matrix(cma_eigen_fx128, 512, EIG_FX_PLAN, fa); break;
        case EK_EIGEN_FX128U: per_matrix(cma_eigen_fx128u, 512, EIG_FX_PLAN, fa); break;
        case EK_EIGEN_R1: per_matrix(cma_eigen_r1, 512, pl_lds, d_, c_, pl_lds, 0); break;
        case EK_EIGEN_R1_FX128: per_matrix(cma_eigen_r1_fx128, 512, EIG_FX_PLAN, fa); break;
        case EK_EIGEN_G1: per_matrix(cma_eigen_g1, 512, pl, d_, c_, pl, 0); break;
        case EK_TRED_MW:
            mw_launched_ = true;
            if (mw_buf_.count != (size_t) c.npop * MW_BUF_DOUBLES) mw_buf_.alloc((size_t) c.npop * MW_BUF_DOUBLES);
            hipLaunchKernelGGL(cma_tred_mw, dim3(8 * MW_G, c.npop), dim3(MW_T), 0, stream_, d_, c_, 0,
                    mw_buf_.p, ++mw_launch_, arg, mw_xcd_);
            break;
        case EK_TRED_TAIL: {   // (n > 256: vectors + a 128 x 130 matrix, the LDS of the plan of 256)
            const EigPlan plt = c.n > 256 ? eig_plan(256, 256) : pl;
            per_matrix(cma_tred_tail, 512, plt, d_, c_, plt, arg);
            break;
        }
        case EK_EIG_HALVES:
            allow_lds((const void*) cma_eig_halves, 160 * 1024 - 768);
            hipLaunchKernelGGL(cma_eig_halves, dim3(3, c.npop), dim3(512), EIG_FX_PLAN.lds_bytes, stream_, d_, c_,
                    EIG_FX_PLAN, pl.lda);
            break;
        case EK_EIGEN_G2: per_matrix(cma_eigen_g2, 512, pl, d_, c_, pl, arg); break;
        case EK_EIG_SECULAR: per_columns(cma_eig_secular, 32, 512); break;
        case EK_EIG_LOWNER: per_columns(cma_eig_lowner, 32, 512); break;
        case EK_EIG_FCOLS: per_columns(cma_eig_fcols, 32, 512); break;
        case EK_EIGEN_G: per_matrix(cma_eigen_g, 512, pl, d_, c_, pl, 0); break;
        case EK_TRED_MW512:
            mw_launched_ = true;
            if (mw_buf_.count != (size_t) c.npop * (mw_buf_doubles(512) + mw_buf_doubles(256)))
                mw_buf_.alloc((size_t) c.npop * (mw_buf_doubles(512) + mw_buf_doubles(256)));
            hipLaunchKernelGGL(cma_tred_mw512, dim3(8 * 16, c.npop), dim3(MW_T), 0, stream_, d_, c_, 0,
                    mw_buf_.p, ++mw_launch_, arg, mw_xcd_);
            break;
        case EK_TRED_MW_CHAIN:
            hipLaunchKernelGGL(cma_tred_mw_chain, dim3(8 * MW_G, c.npop), dim3(MW_T), 0, stream_, d_, c_,
                    mw_buf_.p + (size_t) c.npop * mw_buf_doubles(512), ++mw_launch_, 128, mw_xcd_);
            break;
        case EK_EIGEN_B4: per_matrix(cma_eigen_b4, 512, pl, d_, c_, pl, 0); break;
        case EK_EIGEN_B: per_matrix(cma_eigen_b, 512, pl, d_, c_, pl, 0); break;
        case EK_EIG_GEMM1:
            hipLaunchKernelGGL(cma_eig_gemm1, dim3((c.n + 15) / 16, (c.n + 63) / 64, c.npop), dim3(256), 0,
                    stream_, d_, c_, pl.lda, arg);
            break;
        case EK_EIG_GEMM:
            hipLaunchKernelGGL(cma_eig_gemm, dim3((c.n + 63) / 64, (c.n + 63) / 64, c.npop), dim3(256), 0,
                    stream_, d_, c_, pl.lda, arg);
            break;
        case EK_EIG_WY4: per_columns(cma_eig_wy4, 16, 256, arg); break;
        case EK_EIG_WY4_512: per_columns(cma_eig_wy4_512, 16, 256); break;
        case EK_EIG_WY: per_columns(cma_eig_wy, 64, 256); break;
        case EK_POST: case EK_POST_MFMA: break;      // (r.post: launch_post below, in a slot of its own)
        }
    }
    if (r.timed == r.count) timer_.end(stream_);
    BBO_HIP(hipGetLastError());
    timed(K_POST, [&] {
        if (r.post) launch_post(0);
    });
}

void CmaEngine::launch_history_stop()
{
    timed(K_STOP, [&] {
        if (c_.variant == 3)
            hipLaunchKernelGGL(chol_history_stop, dim3(c_.npop), dim3(256), 0, stream_, d_, c_);
        else
            hipLaunchKernelGGL(cma_history_stop, dim3(c_.npop), dim3(64), 0, stream_, d_, c_);
    });
}

// the compatibility path for arbitrary host objectives: X leaves HBM once per generation
void CmaEngine::host_evaluate()
{
    const CmaConst &c = c_;
    const size_t rows = (size_t) c.npop * c.lambda_pad;
    std::vector<double> xh(rows * c.ld), fh(rows, std::numeric_limits<double>::infinity());
    BBO_HIP(hipStreamSynchronize(stream_));
    X_.download(xh.data(), xh.size());
    std::vector<CmaScal> sc(c.npop);
    scal_.download(sc.data(), c.npop);
    for (int p = 0; p < c.npop; p++) {
        if (c.honor_stop && sc[p].stop) continue;
        const size_t r0 = (size_t) p * c.lambda_pad;
        obj_.eval_host(xh.data() + r0 * c.ld, c.lambda, c.n, c.ld, fh.data() + r0);
        nan_to_inf(fh.data() + r0, c.lambda);
    }
    f_.upload(fh.data(), rows);
}

// an objective program: X is evaluated where it lies, on the engine's stream, nothing is waited for
void CmaEngine::program_evaluate()
{
    prog_.launch(stream_, c_.lambda, c_.honor_stop ? (const void*) &d_.scal->stop : nullptr, (int) sizeof(CmaScal),
            &prog_timer_);
}

// n <= 16, lambda <= 64, on-device objective: whole generations in one launch
// (cma_small_generations).  The per-kernel timers and DBG_NO_SMALL_FUSED keep the nine-kernel
// path, which computes the same bits.
bool CmaEngine::small_fused_ok() const
{
    const CmaConst &c = c_;
    return c.variant < 2 && c.ld == 16 && c.n >= 2 && c.lambda_pad <= 64 && obj_.fused()
            && c.npop <= SMALL_FUSED_MAXP && !timer_.on() && !(d_.dbg & (DBG_NO_EIGEN_SMALL | DBG_NO_SMALL_FUSED));
}

void CmaEngine::launch_small(int gens, bool honor_stop)
{
    small_fused_ = true;
    c_.honor_stop = honor_stop ? 1 : 0;
    c_.use_zn = c_.bound ? 0 : 1;          // cma_sample_eval64 always hands down ||z||^2
    const int ldy = gram_ldy(c_.ld);
    size_t lds = gram_lds_bytes(c_.ld, c_.rps);
    lds = std::max(lds, (size_t) 64 * (c_.ld + 2) * sizeof(double));
    lds = std::max(lds, (size_t) (16 * (c_.ld + 2) + 64) * sizeof(double));
    const int scratch = (int) ((lds + 15) / 16 * 2);                 // doubles, 16-byte aligned
    const size_t total = ((size_t) scratch + small_state_doubles(c_)) * sizeof(double);
    allow_lds((const void*) cma_small_generations, 120 * 1024);
    BBO_REQUIRE(total <= 120 * 1024, "small fused path: state does not fit LDS");
    hipLaunchKernelGGL(cma_small_generations, dim3(c_.npop), dim3(256), total, stream_, d_, c_,
            gens, ldy, scratch);
    BBO_HIP(hipGetLastError());
}

void CmaEngine::generation(bool honor_stop)
{
    if (small_fused_ok()) {
        launch_small(1, honor_stop);
        return;
    }
    small_fused_ = false;
    c_.honor_stop = honor_stop ? 1 : 0;
    launch_sample_eval();
    if (obj_.needs_host()) host_evaluate();
    else if (obj_.is_program()) program_evaluate();
    launch_rank();
    // n = ld = 128 in front of cma_eigen_fx128: that kernel forms C on its load, no cma_cov launch
    // (DBG_COV_UNFUSED keeps the pair; phase() always launches it)
    const EigRoute route = eig_route(true, true);
    launch_update(!route.forms_c);
    launch_eigen(route);
    launch_history_stop();
}

void CmaEngine::phase(int which)
{
    BBO_REQUIRE(inited_, "phase before init");
    BBO_HIP(hipSetDevice(params_.device));
    c_.honor_stop = 0;
    d_.mw_fault = mw_fault_from_env();
    switch (which) {
    case BBO_PHASE_SAMPLE_EVALUATE:
        launch_sample_eval();
        if (obj_.needs_host()) host_evaluate();
        else if (obj_.is_program()) program_evaluate();
        break;
    case BBO_PHASE_RANK: launch_rank(); break;
    case BBO_PHASE_UPDATE: launch_update(); break;
    case BBO_PHASE_EIGEN: launch_eigen(eig_route()); break;
    case BBO_PHASE_HISTORY_STOP: launch_history_stop(); break;
    default: throw Error(BBO_ERR_ARG, "unknown CMA phase");
    }
    BBO_HIP(hipStreamSynchronize(stream_));
    if (mw_check_failed() && which == BBO_PHASE_EIGEN) {
        // the spread reduction gave up: this generation's decomposition by the one-workgroup path
        launch_eigen(eig_route());
        BBO_HIP(hipStreamSynchronize(stream_));
    }
    timer_.collect();
    prog_timer_.collect();
}

void CmaEngine::inject_normals(const double *z, int count)
{
    BBO_REQUIRE(inited_, "inject_normals before init");
    rank_wrote_norms_ = false;
    coef_tab_forget();
    if (!z) {
        d_.zinject = nullptr;
        return;
    }
    const size_t want = (size_t) c_.npop * c_.lambda * c_.n;
    BBO_REQUIRE((size_t) count == want, "inject_normals: count must be populations*lambda*n");
    if (zinject_.count != want) zinject_.alloc(want);
    zinject_.upload(z, want);
    d_.zinject = zinject_.p;
}

// The stamps of cma_rank_sort's coefficient table go back to 'never', in stream order and without a wait:
// a ranking that went before a change of the state from outside does not vouch for an update after it.
void CmaEngine::coef_tab_forget()
{
    if (coef_stamp_.p) BBO_HIP(hipMemsetAsync(coef_stamp_.p, 0, coef_stamp_.count * sizeof(int), stream_));
}

void CmaEngine::after_chunk(bool in_run)
{
    if (in_run) return;      // (run() looks at its next poll: inspect)
    if (mw_check_failed()) {
        // the spread reduction gave up (bbo_eig_mw.hpp): the decomposition this generation was due
        // is not lost -- eigenlastev has not moved, the one-workgroup kernels take it now
        launch_eigen(eig_route());
        BBO_HIP(hipStreamSynchronize(stream_));
    }
}

void CmaEngine::inspect(const std::vector<CmaScal> &sc)
{
    // (the one host-side copy of "every population's C^-1/2 matches its (B, D)": see launch_rank)
    bool stale = false;
    for (const auto &s : sc) stale = stale || !s.basis_ok;
    basis_maybe_stale_ = stale;
    // (bbo_eig_mw.hpp: back to the one-workgroup reduction; the generations since the time-out
    // returned from the spread kernel at entry, the next one decomposes -- eigenlastev stood still)
    mw_check_failed();
    for (const auto &s : sc)
        if (s.eig_mw_fail && !mw_disabled_) {
            mw_disabled_ = true;
            mw_release();
        }
}

// (one launch = `chunk` generations on the fused path: keep a launch to tens of milliseconds
// whatever poll_every says)
int CmaEngine::chunk_limit(int want)
{
    return small_fused_ok() ? std::min(want, 512) : want;
}

void CmaEngine::launch_chunk(int gens)
{
    if (small_fused_ok()) launch_small(gens, true);
    else Engine::launch_chunk(gens);
}

void CmaEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    CmaScal s;
    scal_.download(&s, 1, population);
    std::vector<double> x(c_.ld);
    // bestSolution(), base_cmaes.cpp:232-238: the mean before the first generation, else
    // the best candidate of the LAST generation
    if (s.it <= 0) xmean_.download(x.data(), c_.ld, (size_t) population * c_.ld);
    else X_.download(x.data(), c_.ld, ((size_t) population * c_.lambda_pad + s.ibw[0]) * c_.ld);
    std::copy(x.begin(), x.begin() + c_.n, x_out);
    *n_evals = s.fev;
    // solution() re-runs converged() (base_cmaes.cpp:158-160); before any generation the
    // tests see it = 0 and the initial state
    if (s.it <= 0) {
        // (CholeskyCmaes::converged on the initial state: all f and all radii are 0, both parts hold)
        *converged = c_.variant == 3 ? (c_.tol >= 0. ? 1 : 0) : (0 >= c_.mit) ? 1 : 0;
    } else {
        *converged = s.flag != 0 ? 1 : 0;
    }
}

void CmaEngine::optimize(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj, double *x_out, int *n_evals, int *converged)
{
    init(n, lower, upper, guess, obj);
    // while (_fev < _mfev) { iterate(); if (converged()) break; }   base_cmaes.cpp:166-172
    const int max_gen = c_.mfev / c_.lambda + 2;
    run(max_gen);
    CmaScal s;
    scal_.download(&s, 1, 0);
    std::vector<double> x(c_.ld);
    if (s.it <= 0) xmean_.download(x.data(), c_.ld, 0);
    else X_.download(x.data(), c_.ld, (size_t) s.ibw[0] * c_.ld);
    std::copy(x.begin(), x.begin() + c_.n, x_out);
    *n_evals = s.fev;
    *converged = (s.stop == 1) ? 1 : 0;
}

double CmaEngine::evaluate_point(const double *x)
{
    if (obj_.needs_host()) {
        double f = 0.;
        obj_.eval_host(x, 1, c_.n, c_.n, &f);
        return f;
    }
    if (obj_.is_program()) {
        BBO_HIP(hipSetDevice(params_.device));
        return prog_.evaluate_point(stream_, x);
    }
    // restart drivers re-evaluate one point per restart (bipop_cmaes.cpp:86): host
    // arithmetic with the same definition and the same per-coordinate table
    return builtin_objective_host(obj_.builtin, c_.n, x, aux_h_.data());
}

// ---- named state access ---------------------------------------------------------------
int CmaEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const CmaConst &c = c_;
    const size_t ld = c.ld, n = c.n;
    const StateOut o { out, cap };
    if (c.variant == 2 && (k == "B" || k == "C" || k == "invsqrtC" || k == "ycoeff"))
        throw Error(BBO_ERR_KEY, "SepCMAES keeps a diagonal covariance: read 'csep' and 'D'");
    if (c.variant == 3 && (k == "B" || k == "C" || k == "D" || k == "invsqrtC" || k == "ycoeff" || k == "csep"))
        throw Error(BBO_ERR_KEY, "CholeskyCMAES keeps the factor: read 'A'");
    if (k == "A") {
        if (c.variant != 3) throw Error(BBO_ERR_KEY, "'A' belongs to CholeskyCMAES");
        return o.rows(A_, p * ld, c.n, c.n, c.ld);
    }
    if (k == "xmean") return o.vec(xmean_, p * ld, (int) n);
    if (k == "xold") return o.vec(xold_, p * ld, (int) n);
    if (k == "pc") return o.vec(pc_, p * ld, (int) n);
    if (k == "ps") return o.vec(ps_, p * ld, (int) n);
    if (k == "D") return o.vec(D_, p * ld, (int) n);
    if (k == "csep") return o.vec(csep_, p * ld, (int) n);
    if (k == "B") return o.rows(B_, p * ld, c.n, c.n, c.ld);
    if (k == "C") return o.rows(C_, p * ld, c.n, c.n, c.ld);
    if (k == "invsqrtC") {
        if (c.lazy_isc && out) {         // not kept current by the generations: form it now
            const int hs = c_.honor_stop;
            c_.honor_stop = 0;
            launch_post(3);
            c_.honor_stop = hs;
            BBO_HIP(hipGetLastError());
            BBO_HIP(hipStreamSynchronize(stream_));
        }
        return o.rows(isc_, p * ld, c.n, c.n, c.ld);
    }
    if (k == "BD") {
        // the sampler's operand B diag(D) as the kernels hold it (bfrag_index), unpacked to n x n row-major
        if (out && cap >= (int) (n * n)) {
            std::vector<double> pk(ld * ld);
            BDp_.download(pk.data(), ld * ld, p * ld * ld);
            for (size_t i = 0; i < n; i++)
                for (size_t j = 0; j < n; j++) out[i * n + j] = pk[bfrag_index(i, j, ld)];
        }
        return (int) (n * n);
    }
    if (k == "arx") return o.rows(X_, (size_t) p * c.lambda_pad, c.lambda, c.n, c.ld);
    if (k == "weights") {
        if (out && cap >= c.mu) weights_.download(out, c.mu);
        return c.mu;
    }
    if (k == "fitness") {
        if (out && cap >= c.lambda) f_.download(out, c.lambda, (size_t) p * c.lambda_pad);
        return c.lambda;
    }
    if (k == "fit_idx" || k == "fit_val" || k == "rank") {
        if (out && cap >= c.lambda) {
            std::vector<int> ord(c.lambda);
            (k == "rank" ? rank_ : order_).download(ord.data(), c.lambda,
                    (size_t) p * c.lambda_pad);
            if (k == "fit_val") {
                std::vector<double> f(c.lambda);
                f_.download(f.data(), c.lambda, (size_t) p * c.lambda_pad);
                for (int i = 0; i < c.lambda; i++) out[i] = f[ord[i]];
            } else {
                for (int i = 0; i < c.lambda; i++) out[i] = ord[i];
            }
        }
        return c.lambda;
    }
    if (k == "ycoeff") {
        if (out && cap >= c.mu) {
            std::vector<double> S(c.mu_pad);
            S_.download(S.data(), c.mu_pad, (size_t) p * c.mu_pad);
            for (int i = 0; i < c.mu; i++) out[i] = S[i] / std::max(S[c.mu - 1 - i], 1e-8);
        }
        return c.mu;
    }
    if (k == "S") {          // the whitened squared norms of the worst mu, as the last ranking or update left them
        if (c.variant != 1) throw Error(BBO_ERR_KEY, "'S' belongs to ActiveCMAES");
        if (out && cap >= c.mu) S_.download(out, c.mu, (size_t) p * c.mu_pad);
        return c.mu;
    }
    if (k == "zn2") {        // ||z||^2 of every candidate, where the last sampler handed it down (else stale)
        if (!zn2_.p) return 0;
        if (out && cap >= c.lambda) zn2_.download(out, c.lambda, (size_t) p * c.lambda_pad);
        return c.lambda;
    }
    if (k == "zlast") {
        const size_t cnt = (size_t) c.lambda * n;
        if (!zrecord_.p) return 0;
        if (out && cap >= (int) cnt) zrecord_.download(out, cnt, p * cnt);
        return (int) cnt;
    }
    if (k == "profile") return profile_report(out, cap);
    if (const int r = prog_get(k, out, cap); r >= 0) return r;
    if (k == "eig_work") {   // diagnostic: the eigensolver's global scratch of population p
        const size_t cnt = std::min((size_t) 4 * eig_slab(c.ld), eig_work_.count);
        if (out && (size_t) cap >= cnt) eig_work_.download(out, cnt, (size_t) p * 4 * eig_slab(c.ld));
        return (int) cnt;
    }
    if (k == "eig_stamps") {
        if (!stamps_.p) return 0;
        if (out && cap >= 48) {
            long long t[48];
            stamps_.download(t, 48);
            for (int i = 0; i < 48; i++) out[i] = (double) t[i];
        }
        return 48;
    }
    if (k == "best_hist" || k == "kth_hist") {
        if (out && cap >= c.hlen)
            (k == "best_hist" ? hist_best_ : hist_kth_).download(out, c.hlen, (size_t) p * c.hlen);
        return c.hlen;
    }
    CmaScal s;
    scal_.download(&s, 1, p);
    if (k == "sigma") return o.one(s.sigma);
    if (k == "it") return o.one(s.it);
    if (k == "fev") return o.one(s.fev);
    if (k == "flag") return o.one(s.flag);
    if (k == "stop") return o.one(s.stop);
    if (k == "hsig") return o.one(s.hsig);
    if (k == "pslen") return o.one(s.pslen);
    if (k == "fbest") return o.one(s.fbest);
    if (k == "fworst") return o.one(s.fworst);
    if (k == "eigenlastev") return o.one(s.eigenlastev);
    if (k == "eigen_done") return o.one(s.eigen_done);
    if (k == "basis_ok") return o.one(s.basis_ok);
    if (k == "eig_stage") return o.one(s.eig_stage);
    if (k == "eig_mw_fail") return o.one(s.eig_mw_fail);     // (bbo_eig_mw.hpp: sticky)
    if (k == "chol_repairs") {                             // (chol_factor: sticky)
        if (c.variant != 3) throw Error(BBO_ERR_KEY, "'chol_repairs' belongs to CholeskyCMAES");
        int r = 0;
        chol_repairs_.download(&r, 1, p);
        return o.one(r);
    }
    if (c.variant == 3 && k == "chol_tri") return o.one(chol_tri_ ? 1 : 0);
    if (c.variant == 3 && k == "stol") return o.one(c.stol);
    if (c.variant == 3 && k == "ranked") return o.one(c.ranked);
    if (k == "eig_mw_off") return o.one(mw_disabled_ ? 1 : 0);
    if (k == "eig_split_maxp") return o.one(split_maxp_);
    if (k == "eig_fixed128") return o.one(last_route_.fixed ? 1 : 0);     // the last decomposition took a fixed-shape kernel
    if (k == "cov_fused") return o.one(last_route_.forms_c ? 1 : 0);      // the last generation formed C inside it
    if (k == "eig_route") {                                               // its kernels in launch order: EigKernel ids
        double ids[sizeof(last_route_.step) / sizeof(last_route_.step[0])];
        for (int i = 0; i < last_route_.count; i++) ids[i] = last_route_.step[i].k;
        return o.copy(ids, last_route_.count);
    }
    if (k == "rank_route") return o.one(last_rank_);                      // the form of the last launch_rank: RankKernel
    if (k == "sample_route") return o.one(last_sample_.k);                // the last launch_sample_eval: SampleKernel, -1 before any
    if (k == "sample_lean") return o.one(last_sample_.full);              // ... took a lean build
    if (k == "sample_transposed") return o.one(last_sample_.transposed);  // ... and the transposed tile loop
    if (k == "sample128_rowlayout") return o.one(sample128_rowlayout_ ? 1 : 0);
    if (k == "update_route") {                                            // the last launch_update in launch order: UpdateKernel ids
        double ids[sizeof(last_update_.step) / sizeof(last_update_.step[0])];
        for (int i = 0; i < last_update_.count; i++) ids[i] = last_update_.step[i].k;
        return o.copy(ids, last_update_.count);
    }
    if (k == "small_fused") return o.one(small_fused_ ? 1 : 0);           // the last generation or chunk ran in cma_small_generations
    if (k == "splits") return o.one(c.splits);                            // Gram slabs per population
    if (k == "gram_coef_stamp") {      // it + 1 of the last generation whose cma_rank_sort left cma_gram128s its
                                       // coefficient table: equal to "it" after a generation that took the table, 0 = never
        int stamp = 0;
        if (coef_stamp_.p) coef_stamp_.download(&stamp, 1, p);
        return o.one(stamp);
    }
    if (k == "eig_mw_reserved") return o.one((double) mw_reserved_);       // this engine's share of the device's ...
    if (k == "eig_mw_capacity") {                                        // ... budget of spread workgroups
        MwBudget &b = MwBudget::get();
        std::lock_guard<std::mutex> lock(b.m);
        return o.one((double) b.capacity(params_.device));
    }
    if (k == "best_len") return o.one(s.hist_len);
    if (k == "best_buffer") return o.one(s.hist_head);
    if (k == "ibest") return o.one(s.ibw[0]);
    if (k == "ybw") return o.copy(s.ybw, 4);    // best, 2nd best, 2nd worst, worst of the last ranking ...
    if (k == "ibw") {                           // ... and their candidates
        const double ids[4] = { (double) s.ibw[0], (double) s.ibw[1], (double) s.ibw[2], (double) s.ibw[3] };
        return o.copy(ids, 4);
    }
    if (k == "n") return o.one(c.n);
    if (k == "lambda") return o.one(c.lambda);
    if (k == "mu") return o.one(c.mu);
    if (k == "mueff") return o.one(c.mueff);
    if (k == "cc") return o.one(c.cc);
    if (k == "cs") return o.one(c.cs);
    if (k == "c1") return o.one(c.c1);
    if (k == "cmu") return o.one(c.cmu);
    if (k == "cneg") return o.one(c.cneg);
    if (k == "alphaold") return o.one(c.alphaold);
    if (k == "cm") return o.one(c.cm);
    if (k == "ccov") return o.one(c.ccov);
    if (k == "damps") return o.one(c.damps);
    if (k == "chi") return o.one(c.chi);
    if (k == "eigenfreq") return o.one(c.eigenfreq);
    if (k == "hlen") return o.one(c.hlen);
    if (k == "ik") return o.one(c.ik);
    if (k == "mit") return o.one(c.mit);
    if (k == "mfev") return o.one(c.mfev);
    if (k == "sigma0") return o.one(c.sigma0);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int CmaEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    rank_wrote_norms_ = false;      // (S of a ranking before this call may not match the new state)
    coef_tab_forget();              // (nor its coefficient table)
    const CmaConst &c = c_;
    const size_t ld = c.ld, n = c.n;
    auto vec_in = [&](DevBuf<double> &b) {          // n -> [P][ld]
        BBO_REQUIRE(count == (int) n, "set: wrong element count");
        upload_rows(b, p, 1, c.n, c.ld, in);
        return count;
    };
    auto mat_in = [&](DevBuf<double> &b) {          // [n][n] -> [ld][ld]: the padding ROWS are zeroed too
        BBO_REQUIRE(count == (int) (n * n), "set: wrong element count");
        std::vector<double> tmp(ld * ld, 0.);
        for (size_t i = 0; i < n; i++) std::copy(in + i * n, in + (i + 1) * n, tmp.begin() + i * ld);
        b.upload(tmp.data(), ld * ld, p * ld * ld);
        return count;
    };
    if (c.variant == 2 && (k == "B" || k == "C" || k == "D"))
        throw Error(BBO_ERR_KEY, "SepCMAES: set 'csep' (D is its square root)");
    if (c.variant == 3 && (k == "B" || k == "C" || k == "D" || k == "csep"))
        throw Error(BBO_ERR_KEY, "CholeskyCMAES keeps the factor: set 'A'");
    if (k == "A") {
        // the factor and its packed form for the sampler (upper triangle dropped)
        if (c.variant != 3) throw Error(BBO_ERR_KEY, "'A' belongs to CholeskyCMAES");
        BBO_REQUIRE(count == (int) (n * n), "set: wrong element count");
        std::vector<double> a(ld * ld, 0.), pk(ld * ld, 0.);
        for (size_t i = 0; i < n; i++)
            for (size_t j = 0; j <= i; j++) {
                a[i * ld + j] = in[i * n + j];
                pk[bfrag_index(i, j, ld)] = in[i * n + j];
            }
        A_.upload(a.data(), ld * ld, p * ld * ld);
        BDp_.upload(pk.data(), ld * ld, p * ld * ld);
        return count;
    }
    if (c.variant == 3 && k == "arx") {          // (crafted stop states of the Cholesky variant's rule)
        BBO_REQUIRE(count == (int) (c.lambda * n), "set: wrong element count");
        upload_rows(X_, (size_t) p * c.lambda_pad, c.lambda, c.n, c.ld, in);
        return count;
    }
    if (k == "fitness") {      // (crafted states; the ranking is NOT redone: fit_idx keeps its order.  NaN
                               // goes in as +inf, like every evaluation path: no NaN reaches a ranking)
        BBO_REQUIRE(count == c.lambda, "set: wrong element count");
        std::vector<double> f(in, in + c.lambda);
        nan_to_inf(f.data(), c.lambda);
        f_.upload(f.data(), c.lambda, (size_t) p * c.lambda_pad);
        return count;
    }
    if (k == "xmean") return vec_in(xmean_);
    if (k == "xold") return vec_in(xold_);
    if (k == "pc") return vec_in(pc_);
    if (k == "ps") return vec_in(ps_);
    if (k == "csep") {
        BBO_REQUIRE(c.variant == 2, "csep belongs to SepCMAES");
        const int r = vec_in(csep_);
        std::vector<double> dd(ld, 1.);
        for (size_t i = 0; i < n; i++) dd[i] = std::sqrt(in[i]);
        D_.upload(dd.data(), ld, p * ld);
        return r;
    }
    if (k == "C") return mat_in(C_);
    if (k == "best_hist" || k == "kth_hist") {   // cmaes_history rings (crafted stop states)
        BBO_REQUIRE(count == c.hlen, "set: wrong element count");
        (k == "best_hist" ? hist_best_ : hist_kth_).upload(in, c.hlen, (size_t) p * c.hlen);
        return count;
    }
    if (k == "invsqrtC") throw Error(BBO_ERR_KEY, "invsqrtC is derived from B and D: set those");
    if (k == "B" || k == "D") {
        int r;
        if (k == "D") {
            BBO_REQUIRE(count == (int) n, "set: wrong element count");
            std::vector<double> tmp(ld, 1.);
            std::copy(in, in + n, tmp.begin());
            D_.upload(tmp.data(), ld, p * ld);
            r = count;
        } else {
            r = mat_in(B_);
        }
        // refresh C^-1/2 and the packed MFMA operands
        c_.honor_stop = 0;
        launch_post(1);
        BBO_HIP(hipGetLastError());
        BBO_HIP(hipStreamSynchronize(stream_));
        return r;
    }
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (const int r = prog_set(k, in, count); r >= 0) return r;
    if (k == "dbg") {
        d_.dbg = (int) in[0];
        return 1;
    }
    if (c.variant == 3 && k == "chol_tri") {   // n = 128: 1 = the triangular samplers, 0 = the full-operand ones (same bits)
        chol_tri_ = in[0] != 0.;
        return 1;
    }
    if (k == "sample_wide_max") {  // (tuning: at most this many 16-row tiles take the tile-per-workgroup sampler)
        sample_wide_max_tiles_ = (long) in[0];
        return 1;
    }
    if (k == "sample128_rowlayout") {   // 1 = cma_sample_eval128's row-layout tile loop, 0 = the transposed one (same bits)
        sample128_rowlayout_ = in[0] != 0.;
        return 1;
    }
    if (k == "sample128_min") {    // (tuning: candidates in flight from which cma_sample_eval128 draws)
        sample128_min_rows_ = (long) in[0];
        return 1;
    }
    if (k == "eig_split_maxp") {   // (tuning: at most this many populations take the split 64 < n <= 128 decomposition)
        split_maxp_ = (int) in[0];
        return 1;
    }
    if (k == "stop_off") {     // (extension) bit k silences the stop test with flag k
        c_.stop_off = (int) in[0];
        return 1;
    }
    if (k == "ftarget") {      // (extension) f_best <= ftarget stops with flag 10
        c_.ftarget = in[0];
        return 1;
    }
    if (k == "eig_stamps") {
        if (stamps_.count != 48) stamps_.alloc(48);    // [32..47]: step clocks of diagnostic builds
        BBO_HIP(hipStreamSynchronize(stream_));
        BBO_HIP(hipMemset(stamps_.p, 0, 48 * sizeof(long long)));     // (set again = clear)
        d_.stamps = stamps_.p;
        return 1;
    }
    if (k == "record_normals") {
        BBO_REQUIRE(count == 1, "set: wrong element count");
        if (in[0] != 0.) {
            const size_t want = (size_t) c.npop * c.lambda * n;
            if (zrecord_.count != want) zrecord_.alloc(want);
            d_.zrecord = zrecord_.p;
        } else {
            d_.zrecord = nullptr;
        }
        return 1;
    }
    BBO_REQUIRE(count == 1, "set: wrong element count");
    CmaScal s;
    scal_.download(&s, 1, p);
    if (k == "sigma") s.sigma = in[0];
    else if (k == "it") s.it = (int) in[0];
    else if (k == "fev") s.fev = (int) in[0];
    else if (k == "eigenlastev") s.eigenlastev = (int) in[0];
    else if (k == "fbest") s.fbest = in[0];
    else if (k == "fworst") s.fworst = in[0];
    else if (k == "stop") s.stop = (int) in[0];
    else if (k == "best_len") s.hist_len = (int) in[0];
    else if (k == "best_buffer") s.hist_head = (int) in[0];
    else throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
    scal_.upload(&s, 1, p);
    return 1;
}

// The eigensolver for an engine that is not CMA-ES (ACD, bbo_acd.hpp): the one-workgroup decomposition,
// n <= 128 with the matrix in LDS, of every matrix of the view d, c whose CmaScal says it is due.  The
// kernels are the ones launch_eigen uses for a batch (EK_EIGEN_128, EK_EIGEN_256, EK_EIGEN); the view needs
// C, B, D, eig_work (eigen_view_scratch doubles a matrix) and scal, lazy_isc = 0 and no diagnostics.
size_t eigen_view_scratch(int ld)
{
    return 4 * eig_slab(ld);
}

void launch_eigen_view(hipStream_t stream, const CmaDev &d, const CmaConst &c)
{
    const EigPlan pl = eig_plan(c.n, c.ld);
    if (!pl.use_lds || !pl.reg_path || c.lazy_isc || d.dbg || d.stamps)
        throw Error(BBO_ERR_ARG, "launch_eigen_view: n <= 128, no lazy_isc, no diagnostics");
    auto per_matrix = [&](auto kernel, int threads) {
        allow_lds((const void*) kernel, 160 * 1024 - 768);
        hipLaunchKernelGGL(kernel, dim3(c.npop), dim3(threads), pl.lds_bytes, stream, d, c, pl, 0);
    };
    if (pl.threads == 128) per_matrix(cma_eigen_128, 128);
    else if (pl.threads == 256) per_matrix(cma_eigen_256, 256);
    else per_matrix(cma_eigen, 512);
}

} // namespace bbo
