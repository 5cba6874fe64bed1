// bbo_bh.hip -- host side of the BasinHopping engine.  Reference behaviour restated on the host:
// BasinHopping::BasinHopping / init / optimize (basinhopping.cpp:109-153, :196-203) and the table it prints.
#include "bbo_bh_kernels.hpp"
#include "bbo_tabular.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_INNER = 0, K_HOP, K_COLLECT, K_DECIDE, K_BEGIN, K_EVALUATE, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:bh_inner_walk", "bbo:bh_hop", "bbo:bh_collect", "bbo:bh_decide",
        "bbo:bh_begin", "bbo:bh_evaluate" };
constexpr int BH_DEFAULT_POLL = 8;       // rounds of (walk chunk, hop) between polls of the finished chains
const std::vector<int> BH_WIDTHS = { 5, 25, 5, 25, 6, 25, 10 };      // basinhopping.cpp:148
}

void bh_draws_host(uint64_t seed, int substream, int hop, int n, double *out)
{
    for (int j = 0; j < n; j++) out[j] = bh_step_uniform(seed, (uint32_t) substream, (uint32_t) hop, (uint32_t) j);
    out[n] = bh_accept_uniform(seed, (uint32_t) substream, (uint32_t) hop);
}

BhEngine::BhEngine(const bbo_params &p, Optimizer *minimizer) :
        params_(p), min_(minimizer)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_BASIN_HOPPING, "BhEngine: bad algo");
    nm_ = dynamic_cast<NmEngine*>(minimizer);
    rosen_ = dynamic_cast<RosenEngine*>(minimizer);
    BBO_REQUIRE(nm_ || rosen_, "BasinHopping: the minimizer must be a NelderMead or a Rosenbrock handle of this library");
    const bbo_params &mp = nm_ ? nm_->params_ : rosen_->params_;
    BBO_REQUIRE(p.populations >= 1 && mp.populations == p.populations,
            "BasinHopping: the minimizer must hold as many populations as there are chains (populations)");
    BBO_REQUIRE(mp.device == p.device, "BasinHopping: the minimizer must live on the same device");
    require_native_minimizer();
    stream_ = nm_ ? nm_->stream_ : rosen_->stream_;
    bbo_bh_params_default(&bp_);
}

BhEngine::~BhEngine()
{
}

// NelderMead(minit = random) addresses its Philox draws by `restarts` alone: every hop would draw the same simplex
void BhEngine::require_native_minimizer() const
{
    BBO_REQUIRE(!nm_ || nm_->np_.minit != 3,
            "BasinHopping: NelderMead(minit=random) draws its simplex by the restart count alone, the same one on "
            "every hop: use another minit");
}

void BhEngine::configure(const bbo_bh_params &bp)
{
    // (legal at any time: a strategy object that has been used is handed over again before the next bbo_init)
    BBO_REQUIRE(std::isfinite(bp.stepsize), "BasinHopping: stepsize must be finite");
    BBO_REQUIRE(bp.adaptive == 0 || bp.adaptive == 1, "BasinHopping: adaptive is 0 or 1");
    BBO_REQUIRE(bp.interval >= 1, "BasinHopping: interval must be >= 1");
    BBO_REQUIRE(std::isfinite(bp.factor) && bp.factor > 0., "BasinHopping: factor must be finite and positive");
    BBO_REQUIRE(bp.accept_rate == bp.accept_rate, "BasinHopping: accept_rate must not be NaN");
    BBO_REQUIRE(bp.temp >= 0., "BasinHopping: temp must be >= 0 (and not NaN)");
    BBO_REQUIRE(bp.mit >= 0, "BasinHopping: mit must be >= 0");
    BBO_REQUIRE(bp.lockstep >= -1 && bp.lockstep <= 1, "BasinHopping: lockstep is 1, 0 or -1 (the engine chooses)");
    BBO_REQUIRE(bp.substream >= 0 && bp.substream < (1 << 24), "BasinHopping: substream must be in [0, 2^24)");
    BBO_REQUIRE(bp.nstep0 >= 0 && bp.naccept0 >= 0, "BasinHopping: nstep0 and naccept0 must be >= 0");
    bp_ = bp;
}

void BhEngine::enter(const char *call, int population)
{
    if (!inited_) throw Error(BBO_ERR_STATE, std::string(call) + " before initialize()");
    BBO_REQUIRE(population >= 0 && population < params_.populations, "population index out of range");
    // the kernels index the minimiser's buffers with this engine's n and ld: a minimiser that was initialised again
    // behind this handle (another problem, or a run of its own) no longer holds the chains' minimisations
    if ((nm_ ? nm_->inits_ : rosen_->inits_) != inner_inits_)
        throw Error(BBO_ERR_STATE, "BasinHopping: the minimizer was initialised again since bbo_init: call bbo_init");
    BBO_HIP(hipSetDevice(params_.device));
    BBO_HIP(hipStreamSynchronize(stream_));
}

template<class Launch>
void BhEngine::timed(int slot, Launch launch)
{
    timer_.begin(stream_, slot);
    launch();
    timer_.end(stream_);
    BBO_HIP(hipGetLastError());
}

void BhEngine::init(int n, const double *lower, const double *upper, const double *guess, const ObjectiveSpec &obj)
{
    inited_ = false;
    if (obj.is_program())
        throw Error(BBO_ERR_ARG, "BasinHopping: objective programs are not supported: its minimizers (NelderMead, "
                "Rosenbrock) refuse them");
    BBO_REQUIRE(n >= 1 && n <= BH_MAX_N, "BasinHopping: dimension must be in [1, 128]");
    for (int j = 0; j < n; j++)
        BBO_REQUIRE(std::isfinite(lower[j]) && std::isfinite(upper[j]),
                "BasinHopping: a step is a fraction of upper - lower: the bounds must be finite");
    require_native_minimizer();
    const int P = params_.populations;
    BBO_REQUIRE(P <= (1 << 24) - bp_.substream, "BasinHopping: substream + populations must be <= 2^24");
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    // the first minimisation starts at the guess (:134); NelderMead builds and values its first simplex here
    min_->init(n, lower, upper, guess, obj);
    inner_inits_ = nm_ ? nm_->inits_ : rosen_->inits_;

    BhConst &c = c_;
    c = BhConst {};
    c.n = n;
    c.ld = round_up(n, 2);
    c.npop = P;
    c.mit = bp_.mit;
    c.substream = bp_.substream;
    c.adaptive = bp_.adaptive;
    c.interval = bp_.interval;
    c.accept_rate = bp_.accept_rate;
    c.factor = bp_.factor;
    c.beta = bp_.temp == 0. ? std::numeric_limits<double>::infinity() : 1. / bp_.temp;      // :96-102
    c.seed = params_.seed;
    // Measured: asynchronous hops are faster at n = 32 with 1, 256 and 4096 chains and at
    // n = 128 with one; at n = 128 with 256 and with 4096 chains lockstep is 4 to 8 % faster.  Between 1 and 256
    // chains and between n = 32 and 128 nothing was measured: the switch is put past one wavefront and at 256.
    lockstep_ = bp_.lockstep >= 0 ? bp_.lockstep != 0 : (n > 64 && P >= 256);

    const size_t ld = c.ld, vec = (size_t) P * ld, rows = (size_t) P * (c.mit + 1);
    x_.alloc(vec); xbest_.alloc(vec); xtrial_.alloc(vec); xsol_.alloc(vec);
    evalue_.alloc(P);
    log_.alloc(rows * BH_LOG_COLS);
    log_start_.alloc(rows * ld); log_sol_.alloc(rows * ld);
    log_fev_.alloc(rows);
    done_.alloc(1);
    scal_.alloc(P);
    lower_.alloc(ld); upper_.alloc(ld);
    inject_.alloc(0);
    {
        std::vector<double> lo(ld, 0.), up(ld, 0.), xt(vec, 0.);
        std::copy(lower, lower + n, lo.begin());
        std::copy(upper, upper + n, up.begin());
        lower_.upload(lo.data(), ld);
        upper_.upload(up.data(), ld);
        for (int p = 0; p < P; p++) std::copy(guess + (size_t) p * n, guess + (size_t) (p + 1) * n, xt.begin() + p * ld);
        xtrial_.upload(xt.data(), vec);
        // row 0 of every chain's log_start in one strided copy
        BBO_HIP(hipMemcpy2D(log_start_.p, (c.mit + 1) * ld * sizeof(double), xt.data(), ld * sizeof(double),
                ld * sizeof(double), P, hipMemcpyHostToDevice));
        BhScal s0 = {};
        s0.stepsize = bp_.stepsize;     // the caller's strategy object with its history: init() resets none of it
        s0.nstep = bp_.nstep0;
        s0.naccept = bp_.naccept0;
        s0.it = -1;
        s0.stage = BH_WAIT_INNER;
        std::vector<BhScal> sc(P, s0);
        scal_.upload(sc.data(), P);
    }
    BhDev &d = d_;
    d = BhDev {};
    d.x = x_.p; d.xbest = xbest_.p; d.xtrial = xtrial_.p; d.xsol = xsol_.p; d.evalue = evalue_.p;
    d.log = log_.p; d.log_start = log_start_.p; d.log_sol = log_sol_.p; d.log_fev = log_fev_.p;
    d.lower = lower_.p; d.upper = upper_.p;
    d.done = done_.p; d.scal = scal_.p;
    inited_ = true;
    printed_ = 0;
    if (bp_.print) tabular_row(BH_WIDTHS, { "it", "f", "conv", "step", "accept", "f*", "fev" }, true);
    hops(1);
}

void BhEngine::inject_draws(const double *table, int count)
{
    enter("bbo_bh_inject_draws");
    if (!table) {
        d_.inject = nullptr;
        c_.inject_hops = 0;
        return;
    }
    const int per = c_.n + 1;
    BBO_REQUIRE(count >= per && count % per == 0, "bbo_bh_inject_draws: (n + 1) uniforms per hop");
    for (int q = 0; q < count; q++) {
        const bool acc = q % per == c_.n;
        BBO_REQUIRE(table[q] >= (acc ? 0. : -1.) && table[q] < 1.,
                "bbo_bh_inject_draws: the step uniforms lie in [-1, 1), the accept uniform in [0, 1)");
    }
    inject_.alloc(count);
    inject_.upload(table, count);
    d_.inject = inject_.p;
    c_.inject_hops = count / per;
}

// a chunk of the minimiser's walk in every population that has not stopped (a built-in objective)
void BhEngine::launch_inner()
{
    timed(K_INNER, [&] {
        if (nm_) nm_->launch_chunk(nm_->params_.poll_every > 0 ? nm_->params_.poll_every : nm_->default_poll());
        else rosen_->launch_chunk(rosen_->params_.poll_every > 0 ? rosen_->params_.poll_every : rosen_->default_poll());
    });
}

void BhEngine::launch_hop(int mode, int k)
{
    static const int slot_of[] = { K_HOP, K_COLLECT, K_DECIDE, K_BEGIN, K_EVALUATE };
    const int threads = c_.n <= 64 ? 64 : BH_THREADS;
    timed(slot_of[mode], [&] {
        if (nm_)
            hipLaunchKernelGGL(bh_hop<BhNm>, dim3(c_.npop), dim3(threads), 0, stream_, d_, c_, nm_->d_, nm_->c_, mode, k);
        else
            hipLaunchKernelGGL(bh_hop<BhRosen>, dim3(c_.npop), dim3(threads), 0, stream_, d_, c_, rosen_->d_, rosen_->c_,
                    mode, k);
    });
}

// the callable at every pending energy point, in population order, one call each
void BhEngine::host_energies()
{
    BBO_HIP(hipStreamSynchronize(stream_));
    const int P = params_.populations;
    std::vector<BhScal> sc(P);
    scal_.download(sc.data(), P);
    std::vector<double> xh(c_.ld);
    for (int p = 0; p < P; p++) {
        if (!sc[p].pending) continue;
        xsol_.download(xh.data(), c_.ld, (size_t) p * c_.ld);
        double f = 0.;
        obj_.eval_host(xh.data(), 1, c_.n, c_.ld, &f);
        nan_to_inf(&f, 1);
        evalue_.upload(&f, 1, p);
    }
}

bool BhEngine::inner_all_stopped()
{
    BBO_HIP(hipStreamSynchronize(stream_));
    return nm_ ? nm_->all_stopped() : rosen_->all_stopped();
}

int BhEngine::finished()
{
    BBO_HIP(hipStreamSynchronize(stream_));
    timer_.collect();
    int done = 0;
    done_.download(&done, 1);
    print_new_rows();
    return done;
}

// the rows of population 0 the last poll has not seen (basinhopping.cpp:150-151, :186-187)
void BhEngine::print_new_rows()
{
    if (!bp_.print) return;
    BhScal s;
    scal_.download(&s, 1, 0);
    if (s.rows <= printed_) return;
    std::vector<double> lg((size_t) (s.rows - printed_) * BH_LOG_COLS);
    log_.download(lg.data(), lg.size(), (size_t) printed_ * BH_LOG_COLS);
    for (int r = 0; r < s.rows - printed_; r++) {
        const double *g = lg.data() + (size_t) r * BH_LOG_COLS;
        tabular_row(BH_WIDTHS, { tabular_int((long) g[0]), tabular_double(g[1]), tabular_int((long) g[2]),
                tabular_double(g[3]), tabular_int((long) g[4]), tabular_double(g[5]), tabular_int((long) g[6]) }, false);
    }
    printed_ = s.rows;
}

// up to k hops of every chain that has hops left
void BhEngine::hops(int k)
{
    const int P = params_.populations;
    k = std::max(0, std::min(k, c_.mit + 1));
    BBO_HIP(hipMemsetAsync(done_.p, 0, sizeof(int), stream_));
    launch_hop(BH_BEGIN, k);
    if (obj_.needs_host()) {
        // lockstep by construction: the minimiser's own host loop to every population's stop, one batch of
        // energies, the decisions
        for (int pass = 0; finished() < P; pass++) {
            // (every pass completes a hop of every chain that has one left: a pass beyond them is a defect here)
            if (pass > k + 1) throw Error(BBO_ERR_STATE, "BasinHopping: the chains did not reach their goal");
            min_->run(std::numeric_limits<int>::max());
            launch_hop(BH_COLLECT, 0);
            host_energies();
            launch_hop(BH_DECIDE, 0);
        }
        return;
    }
    const int poll = params_.poll_every > 0 ? params_.poll_every : BH_DEFAULT_POLL;
    if (finished() >= P) return;
    // A round advances every walking minimiser by at least one evaluation, and a minimisation ends within its
    // budget and one factorial test or line search past it: more rounds than that is a defect here, reported and
    // never waited for.
    const bbo_params &mp = nm_ ? nm_->params_ : rosen_->params_;
    const long long most = ((long long) k + 1) * ((long long) mp.mfev + 4LL * c_.n + 16) + poll + 2;
    for (long long round = 1;; round++) {
        if (round > most) throw Error(BBO_ERR_STATE, "BasinHopping: the chains did not reach their goal");
        launch_inner();
        if (!lockstep_) {
            launch_hop(BH_FUSED, 0);
            if (round % poll == 0 && finished() >= P) break;
        } else if (inner_all_stopped()) {
            launch_hop(BH_FUSED, 0);
            if (finished() >= P) break;
        }
    }
}

// the hop count of every chain
std::vector<int> BhEngine::hop_counts()
{
    std::vector<BhScal> sc(params_.populations);
    scal_.download(sc.data(), sc.size());
    std::vector<int> its;
    for (const auto &s : sc) its.push_back(s.it);
    return its;
}

void BhEngine::iterate()
{
    enter("iterate()");
    hops(1);
}

int BhEngine::run(int max_hops)
{
    enter("run()");
    const std::vector<int> before = hop_counts();
    hops(std::max(0, std::min(max_hops, c_.mit)));
    const std::vector<int> after = hop_counts();
    int done = 0;       // the hops of the chain that had most left
    for (size_t p = 0; p < after.size(); p++) done = std::max(done, after[p] - before[p]);
    return done;
}

// init(), then hops while it < mit (:196-203)
void BhEngine::optimize(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj, double *x_out, int *n_evals, int *converged)
{
    init(n, lower, upper, guess, obj);
    hops(c_.mit);
    solution(0, x_out, n_evals, converged);
}

// solution() (:192-194): the best, converged = false always
void BhEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter("solution()", population);
    BhScal s;
    scal_.download(&s, 1, population);
    std::vector<double> x(c_.ld);
    xbest_.download(x.data(), c_.ld, (size_t) population * c_.ld);
    std::copy(x.begin(), x.begin() + c_.n, x_out);
    *n_evals = s.fev;
    *converged = 0;
}

// bbo_bh_phase: 0 every idle chain with hops left takes its step and re-arms its minimiser, 1 collect, 2 the
// built-in or the callable at the pending energy points, 3 decide.  The minimiser walks through its own handle.
void BhEngine::phase(int which)
{
    enter("bbo_bh_phase");
    BBO_REQUIRE(which >= 0 && which < 4, "bbo_bh_phase: 0 step, 1 collect, 2 evaluate, 3 decide");
    if (which == 0) {
        BBO_HIP(hipMemsetAsync(done_.p, 0, sizeof(int), stream_));
        launch_hop(BH_BEGIN, 1);
    } else if (which == 1) {
        launch_hop(BH_COLLECT, 0);
    } else if (which == 2) {
        if (obj_.needs_host()) host_energies();
        else launch_hop(BH_EVALUATE, 0);
    } else {
        launch_hop(BH_DECIDE, 0);
    }
    BBO_HIP(hipStreamSynchronize(stream_));
    timer_.collect();
}

int BhEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter("get()", p);
    const BhConst &c = c_;
    BhScal s;
    scal_.download(&s, 1, p);
    const int n = c.n, ld = c.ld;
    const size_t pv = (size_t) p * ld, pr = (size_t) p * (c.mit + 1);
    const StateOut o { out, cap };
    if (k == "profile") return timer_.report(out, cap);
    if (k == "x") return o.vec(x_, pv, n);
    if (k == "xbest") return o.vec(xbest_, pv, n);
    if (k == "xtrial") return o.vec(xtrial_, pv, n);
    if (k == "xsol") return o.vec(xsol_, pv, n);
    if (k == "energy") return o.one(s.energy);
    if (k == "fbest") return o.one(s.bestenergy);
    if (k == "stepsize") return o.one(s.stepsize);
    if (k == "nstep") return o.one(s.nstep);
    if (k == "naccept") return o.one(s.naccept);
    if (k == "it") return o.one(s.it);
    if (k == "fev") return o.one(s.fev);
    if (k == "flag") return o.one(s.it >= c.mit ? 2 : 0);
    if (k == "stage") return o.one(s.stage);
    if (k == "pending") return o.one(s.pending);
    if (k == "log") return o.vec(log_, pr * BH_LOG_COLS, s.rows * BH_LOG_COLS);
    if (k == "log_start") return o.rows(log_start_, pr, s.rows, n, ld);
    if (k == "log_sol") return o.rows(log_sol_, pr, s.rows, n, ld);
    if (k == "log_fev") return o.ints(log_fev_, pr, s.rows);
    if (k == "lockstep") return o.one(lockstep_ ? 1 : 0);
    if (k == "n") return o.one(n);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int BhEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter("set()", p);
    const int n = c_.n;
    if (k == "profile") {
        BBO_REQUIRE(count == 1, "profile: one value");
        timer_.enable(in[0] != 0., K_COUNT, K_NAMES);
        return 1;
    }
    BhScal s;
    scal_.download(&s, 1, p);
    if (k == "x" || k == "energy" || k == "stepsize" || k == "nstep" || k == "naccept") {
        BBO_REQUIRE(s.stage == BH_IDLE, "x, energy, stepsize, nstep, naccept: not while a hop is under way");
        if (k == "x") {
            BBO_REQUIRE(count == n, "x: n values");
            x_.upload(in, n, (size_t) p * c_.ld);
            return count;
        }
        BBO_REQUIRE(count == 1, "energy, stepsize, nstep, naccept: one value");
        if (k == "energy") {
            s.energy = in[0] != in[0] ? std::numeric_limits<double>::infinity() : in[0];
        } else if (k == "stepsize") {
            BBO_REQUIRE(std::isfinite(in[0]), "stepsize: finite");
            s.stepsize = in[0];
        } else {
            BBO_REQUIRE(in[0] == std::floor(in[0]) && in[0] >= 0. && in[0] <= 2147483646., "nstep, naccept: one non-negative integer");
            (k == "nstep" ? s.nstep : s.naccept) = (int) in[0];
        }
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_bh_engine(const bbo_params &p, Optimizer *minimizer)
{
    return new BhEngine(p, minimizer);
}

} // namespace bbo
