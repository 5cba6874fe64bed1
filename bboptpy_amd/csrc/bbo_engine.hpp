// bbo_engine.hpp -- the host lifecycle every engine shares: the device and stream of a handle, the
// box and the objective's table in HBM, the guards of the entry points, and iterate() / run() /
// optimize() as template methods over a handful of hooks.  An engine derives from Engine<its
// per-population scalars>, writes init / generation / solution / get / set around its kernels and
// overrides a hook only where its reference's loop differs (host side).  The engines whose
// generation is a walk from evaluation to evaluation derive from WalkEngine, below.
#pragma once

#include "bbo_common.hpp"
#include "bbo_program.hpp"

#include <algorithm>
#include <cmath>
#include <functional>
#include <limits>

namespace bbo {

// a host objective's NaN ranks last (the device objectives do the same, bbo_objectives.hpp)
inline void nan_to_inf(double *f, int n)
{
    for (int i = 0; i < n; i++)
        if (f[i] != f[i]) f[i] = std::numeric_limits<double>::infinity();
}

// converged() before any generation: the radius spread of the initial swarm, radius[off, off + np)
inline int radius_spread_converged(const DevBuf<double> &radius, size_t off, int np, double tol)
{
    std::vector<double> rad(np);
    radius.download(rad.data(), np, off);
    double mean = 0.;
    for (double r : rad) mean += r;
    mean /= np;
    double m2 = 0.;
    for (double r : rad) m2 += (r - mean) * (r - mean);
    return m2 <= (np - 1) * tol * tol ? 1 : 0;
}

// Where get() puts the values of a key: every member returns the key's count and writes only when
// the caller's buffer takes all of it (a call with out == nullptr asks for the count).
struct StateOut {
    double *out;
    int cap;

    bool fits(int cnt) const { return out && cap >= cnt; }
    int one(double v) const
    {
        if (fits(1)) out[0] = v;
        return 1;
    }
    int copy(const double *v, int cnt) const
    {
        if (fits(cnt)) std::copy(v, v + cnt, out);
        return cnt;
    }
    int vec(const DevBuf<double> &b, size_t off, int cnt) const
    {
        if (fits(cnt) && cnt > 0) b.download(out, cnt, off);
        return cnt;
    }
    int ints(const DevBuf<int> &b, size_t off, int cnt) const
    {
        if (fits(cnt) && cnt > 0) {
            std::vector<int> v(cnt);
            b.download(v.data(), cnt, off);
            std::copy(v.begin(), v.end(), out);
        }
        return cnt;
    }
    // [np][ld] -> [np][n]: np rows of a matrix with leading dimension ld, from its row `row0` on
    int rows(const DevBuf<double> &b, size_t row0, int np, int n, int ld) const
    {
        const int cnt = np * n;
        if (fits(cnt) && cnt > 0) {
            std::vector<double> M((size_t) np * ld);
            b.download(M.data(), M.size(), row0 * ld);
            for (int i = 0; i < np; i++)
                std::copy(M.begin() + (size_t) i * ld, M.begin() + (size_t) i * ld + n, out + (size_t) i * n);
        }
        return cnt;
    }
    // the same in another order: place i takes row order[row0 + i] of the `nrows` rows from row0 on
    int rows_by_slot(const DevBuf<double> &b, const DevBuf<int> &order, size_t row0, int nslots, int nrows,
            int n, int ld) const
    {
        const int cnt = nslots * n;
        if (fits(cnt)) {
            std::vector<int> ord(nslots);
            order.download(ord.data(), nslots, row0);
            std::vector<double> M((size_t) nrows * ld);
            b.download(M.data(), M.size(), row0 * ld);
            for (int i = 0; i < nslots; i++)
                std::copy(M.begin() + (size_t) ord[i] * ld, M.begin() + (size_t) ord[i] * ld + n,
                        out + (size_t) i * n);
        }
        return cnt;
    }
    int vec_by_slot(const DevBuf<double> &b, const DevBuf<int> &order, size_t row0, int nslots, int nrows) const
    {
        if (fits(nslots)) {
            std::vector<int> ord(nslots);
            order.download(ord.data(), nslots, row0);
            std::vector<double> v(nrows);
            b.download(v.data(), nrows, row0);
            for (int i = 0; i < nslots; i++) out[i] = v[ord[i]];
        }
        return nslots;
    }
};

// set() of a row matrix, [np][n] -> [np][ld] from row `row0` on (the padding columns zero); with
// `radius`, the rows' Euclidean norms go to radius[row0, row0 + np)
inline void upload_rows(DevBuf<double> &b, size_t row0, int np, int n, int ld, const double *in,
        DevBuf<double> *radius = nullptr)
{
    std::vector<double> M((size_t) np * ld, 0.), rad(np);
    for (int i = 0; i < np; i++) {
        double ssq = 0.;
        for (int j = 0; j < n; j++) {
            const double v = in[(size_t) i * n + j];
            M[(size_t) i * ld + j] = v;
            ssq += v * v;
        }
        rad[i] = std::sqrt(ssq);
    }
    b.upload(M.data(), M.size(), row0 * ld);
    if (radius) radius->upload(rad.data(), np, row0);
}

// the key width of the slot shuffle (cso_perm): half the bits of np, rounded up
inline int shuffle_key_bits(int np)
{
    int bits = 1;
    while ((1u << bits) < (unsigned) np) bits++;
    return (bits + 1) / 2;
}

// the keys that exist only while the draws of a generation are recorded
inline void require_record(bool record, const std::string &k)
{
    if (!record) throw Error(BBO_ERR_STATE, "'" + k + "' needs record_draws");
}

// set() of a permutation of 0 .. count - 1 that arrives as doubles; `what` is the caller's message
inline std::vector<int> permutation_of(const double *in, int count, const char *what)
{
    std::vector<int> perm(count);
    std::vector<char> seen(count, 0);
    for (int q = 0; q < count; q++) {
        BBO_REQUIRE(in[q] >= 0. && in[q] < count && in[q] == std::floor(in[q]) && !seen[(int) in[q]], what);
        seen[(int) in[q]] = 1;
        perm[q] = (int) in[q];
    }
    return perm;
}

// The two tables of an engine whose draws can be replayed: the one the caller injects instead of the
// generator and the one the kernels record into.  Both have the engine's one table length.
struct DrawTables {
    DevBuf<double> inject, draws;

    void clear()
    {
        inject.alloc(0);
        draws.alloc(0);
    }
    // the caller's table (checked by the engine) in HBM; returns what the kernels read
    const double *load(const double *table, size_t want)
    {
        if (!inject.p) inject.alloc(want);
        inject.upload(table, want);
        return inject.p;
    }
    // set("record_draws"): where the kernels record, null when off
    double *record(bool on, size_t len)
    {
        if (on && !draws.p) {
            draws.alloc(len);
            std::vector<double> z(len, 0.);
            draws.upload(z.data(), len);
        }
        return on ? draws.p : nullptr;
    }
};

// What a population has pending for a host objective: `count` points, rows of ld doubles from
// cand[off] on, whose values go to value[p * count ...] (to value[value_off ...] where the engine's
// batches differ in length).  With `stop_below` the batch is a sequential search: the first value
// below it is the last point the callable sees, the values behind it are +inf.
struct PendingPoints {
    const DevBuf<double> *cand;
    size_t off;
    int count, ld;
    DevBuf<double> *value;
    long long value_off = -1;
    const double *stop_below = nullptr;
};

// Scal: the engine's per-population scalars; the base reads its `stop`, `fev` and `conv` (and
// `pending`, in the engines that call host_evaluate_pending).
template<class Scal>
class Engine: public Optimizer {
public:
    ~Engine() override
    {
        if (stream_) (void) hipStreamDestroy(stream_);
    }

    void iterate() override
    {
        enter("iterate()");
        generation(false);
        BBO_HIP(hipStreamSynchronize(stream_));
        after_chunk(false);
        timer_.collect();
        prog_timer_.collect();
    }

    int run(int max_generations) override
    {
        enter("run()");
        {
            // the references loop `while (_fev < _mfev)`: no generation once the budget is spent
            std::vector<Scal> sc(params_.populations);
            scal_.download(sc.data(), sc.size());
            bool touched = false;
            for (auto &s : sc)
                if (!s.stop && budget_spent(s)) {
                    s.stop = 2;
                    touched = true;
                }
            if (touched) scal_.upload(sc.data(), sc.size());
        }
        const int poll = params_.poll_every > 0 ? params_.poll_every : default_poll();
        int done = 0;
        while (done < max_generations) {
            if (all_stopped()) break;
            // (a host objective is polled every generation; a program like a built-in)
            const int chunk = chunk_limit(obj_.needs_host() ? 1 : std::min(poll, max_generations - done));
            launch_chunk(chunk);
            BBO_HIP(hipStreamSynchronize(stream_));
            after_chunk(true);
            timer_.collect();
            prog_timer_.collect();
            done += chunk;
        }
        return done;
    }

    // init + loop until the algorithm's own stop rule or the evaluation budget
    void optimize(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj, double *x_out, int *n_evals, int *converged) override
    {
        init(n, lower, upper, guess, obj);
        run(std::numeric_limits<int>::max());
        int conv = 0;
        solution(0, x_out, n_evals, &conv);
        Scal s;
        scal_.download(&s, 1, 0);
        *converged = s.stop == 1 ? 1 : 0;
    }

protected:
    // (an engine's own parameter checks run before this one: see the derived constructors)
    explicit Engine(const bbo_params &p) :
            params_(p)
    {
        BBO_REQUIRE(p.populations >= 1, "populations must be >= 1");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            throw Error(BBO_ERR_NO_DEVICE, "no HIP device visible: libbbopt_hip has no CPU path");
        BBO_REQUIRE(p.device >= 0 && p.device < ndev, "device ordinal out of range");
        BBO_HIP(hipSetDevice(p.device));
        BBO_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    }

    // ---- the hooks ----------------------------------------------------------------------------
    virtual void generation(bool honor_stop) = 0;
    // run()'s pre-pass: this population must not take another generation
    virtual bool budget_spent(const Scal &s) const { return s.fev >= params_.mfev; }
    // every poll's download of the scalars, before their stop flags are tested
    virtual void inspect(const std::vector<Scal>&) {}
    virtual int chunk_limit(int want) { return want; }
    // generations between polls when bbo_params::poll_every is 0
    virtual int default_poll() const { return 8; }
    virtual void launch_chunk(int gens)
    {
        for (int g = 0; g < gens; g++) generation(true);
    }
    // behind the synchronisation that ends iterate()'s generation (in_run false) or a chunk of run()
    virtual void after_chunk(bool in_run) { (void) in_run; }

    // ---- guards of the entry points -------------------------------------------------------------
    void enter(const char *call)
    {
        if (!inited_) throw Error(BBO_ERR_STATE, std::string(call) + " before initialize()");
        BBO_HIP(hipSetDevice(params_.device));
    }
    void enter_population(const char *call, int p)
    {
        enter(call);
        BBO_REQUIRE(p >= 0 && p < params_.populations, "population index out of range");
        BBO_HIP(hipStreamSynchronize(stream_));
    }

    // the engines that have no program path yet say which have (the same list, in Python's words:
    // PROGRAM_FAMILIES, bboptpy_amd/multivariate.py)
    void reject_program(const ObjectiveSpec &obj, const char *who) const
    {
        if (obj.is_program())
            throw Error(BBO_ERR_ARG, std::string(who) + ": objective programs are supported by the CMA-ES family "
                    "(CMAES, ActiveCMAES, SepCMAES, CholeskyCMAES, IPOP / BIPOP over them) and the DE family "
                    "(JADE, SHADE, SANSDE), and by PIKAIA");
    }

    // get / set of the keys every program-capable engine shares; < 0: not one of them
    int prog_get(const std::string &k, double *out, int cap) const
    {
        double v;
        if (k == "prog_stage") v = prog_.stage();
        else if (k == "prog_staged") v = prog_.bound() && prog_.staged() ? 1. : 0.;
        else if (k == "prog_stage_max_n") v = PROG_STAGE_MAX_N;
        else if (k == "prog_profile") return prog_timer_.report(out, cap);
        else return -1;
        if (out && cap >= 1) out[0] = v;
        return 1;
    }
    int prog_set(const std::string &k, const double *in, int count)
    {
        if (k != "prog_stage") return -1;
        BBO_REQUIRE(count == 1 && (in[0] == -1. || in[0] == 0. || in[0] == 1.),
                "prog_stage: -1 (automatic), 0 (direct) or 1 (staged)");
        prog_.set_stage((int) in[0]);
        return 1;
    }

    void require_finite_box(const char *msg, int n, const double *lower, const double *upper) const
    {
        for (int j = 0; j < n; j++)
            BBO_REQUIRE(std::isfinite(lower[j]) && std::isfinite(upper[j]), msg);
    }

    // the box and the objective's per-coordinate table, padded to ld, on the host and in HBM
    void upload_box(int n, int ld, const double *lower, const double *upper, const ObjectiveSpec &obj)
    {
        lower_h_.assign(ld, 0.);
        upper_h_.assign(ld, 0.);
        aux_h_.assign(ld, 0.);
        std::copy(lower, lower + n, lower_h_.begin());
        std::copy(upper, upper + n, upper_h_.begin());
        fill_objective_aux(obj.fused() ? obj.builtin : -1, n, aux_h_.data());
        lower_.alloc(ld);
        upper_.alloc(ld);
        aux_.alloc(ld);
        lower_.upload(lower_h_.data(), ld);
        upper_.upload(upper_h_.data(), ld);
        aux_.upload(aux_h_.data(), ld);
    }

    // solution(): the row at b[off, off + n), the evaluations and the stop rule's verdict
    void report_solution(const Scal &s, const DevBuf<double> &b, size_t off, int n, int ld, double *x_out,
            int *n_evals, int *converged) const
    {
        std::vector<double> x(ld);
        b.download(x.data(), ld, off);
        std::copy(x.begin(), x.begin() + n, x_out);
        *n_evals = s.fev;
        *converged = s.conv;
    }

    // A host objective over the rows of src ([P][np][ld]), the values to dst ([P][np]); a stopped
    // population is left out under honor_stop.  Without `order` a population is one call of
    // eval_host in row order; with it (slot -> row) the rows are evaluated one by one in slot
    // order, the slots that `skip` names keeping the value dst holds.  Either way the callable is
    // called in the reference's order and exactly `fev` times.
    void host_evaluate_rows(const DevBuf<double> &src, DevBuf<double> &dst, int np, int n, int ld,
            bool honor_stop, const DevBuf<int> *order = nullptr,
            const std::function<bool(int)> &skip = nullptr)
    {
        if (!order) {
            host_evaluate_range(src, dst, 0, params_.populations, np, 0, np, n, ld, honor_stop);
            return;
        }
        BBO_HIP(hipStreamSynchronize(stream_));
        const int P = params_.populations;
        std::vector<Scal> sc(P);
        scal_.download(sc.data(), P);
        std::vector<double> xh((size_t) np * ld), fh(np);
        std::vector<int> occ(np);
        for (int p = 0; p < P; p++) {
            if (honor_stop && sc[p].stop) continue;
            src.download(xh.data(), xh.size(), (size_t) p * np * ld);
            if (skip) dst.download(fh.data(), np, (size_t) p * np);
            order->download(occ.data(), np, (size_t) p * np);
            for (int s = 0; s < np; s++) {
                if (skip && skip(s)) continue;
                const int row = occ[s];
                double f = 0.;
                obj_.eval_host(xh.data() + (size_t) row * ld, 1, n, ld, &f);
                nan_to_inf(&f, 1);
                fh[row] = f;
            }
            dst.upload(fh.data(), np, (size_t) p * np);
        }
    }

    // The same in row order for the populations [p0, p0 + pcount) only, of each the rows [r0, r1) of
    // the `nrows` it holds in src ([P][nrows][ld]) and dst ([P][nrows]): one call of eval_host per
    // population (an engine's initial points, or the points set("x") replaced in one population).
    void host_evaluate_range(const DevBuf<double> &src, DevBuf<double> &dst, int p0, int pcount, int nrows,
            int r0, int r1, int n, int ld, bool honor_stop = false)
    {
        BBO_HIP(hipStreamSynchronize(stream_));
        std::vector<Scal> sc(params_.populations);
        scal_.download(sc.data(), sc.size());
        const int cnt = r1 - r0;
        std::vector<double> xh((size_t) cnt * ld), fh(cnt);
        for (int p = p0; p < p0 + pcount; p++) {
            if (honor_stop && sc[p].stop) continue;
            src.download(xh.data(), xh.size(), ((size_t) p * nrows + r0) * ld);
            obj_.eval_host(xh.data(), cnt, n, ld, fh.data());
            nan_to_inf(fh.data(), cnt);
            dst.upload(fh.data(), cnt, (size_t) p * nrows + r0);
        }
    }

    // A host objective over the points the populations have pending (Scal::pending), in population
    // order, each point one call of eval_host: the callable is called exactly `fev` times.  `points`
    // (p, scalars of p) names them; a stopped population is left out under honor_stop.
    template<class Points>
    void host_evaluate_pending(bool honor_stop, Points points)
    {
        BBO_HIP(hipStreamSynchronize(stream_));
        const int P = params_.populations, n = dimension();
        std::vector<Scal> sc(P);
        scal_.download(sc.data(), P);
        std::vector<double> xh, fh;
        for (int p = 0; p < P; p++) {
            if (!sc[p].pending || (honor_stop && sc[p].stop)) continue;
            const PendingPoints pt = points(p, sc[p]);
            xh.resize((size_t) pt.count * pt.ld);
            fh.assign(pt.count, 0.);
            pt.cand->download(xh.data(), xh.size(), pt.off);
            for (int i = 0; i < pt.count; i++) {
                obj_.eval_host(xh.data() + (size_t) i * pt.ld, 1, n, pt.ld, &fh[i]);
                if (pt.stop_below && fh[i] < *pt.stop_below) {
                    std::fill(fh.begin() + i + 1, fh.end(), std::numeric_limits<double>::infinity());
                    break;
                }
            }
            nan_to_inf(fh.data(), pt.count);
            pt.value->upload(fh.data(), pt.count, pt.value_off >= 0 ? (size_t) pt.value_off : (size_t) p * pt.count);
        }
    }

    // the launches of one slot of get("profile"): `launch` holds the hipLaunchKernelGGLs, with the
    // allow_lds calls and the choice of the kernel, and nothing that waits for the host
    template<class Launch>
    void timed(int slot, Launch launch)
    {
        timer_.begin(stream_, slot);
        launch();
        timer_.end(stream_);
        BBO_HIP(hipGetLastError());
    }

    // One part of a generation on its own, what an engine's bbo_<engine>_phase runs: `part` clears the
    // engine's honor_stop and launches part `which` of the `count`; `call` and `usage` are the
    // engine's own texts.
    template<class Part>
    void run_phase(const char *call, int which, int count, const std::string &usage, Part part)
    {
        enter(call);
        BBO_REQUIRE(which >= 0 && which < count, usage);
        part();
        BBO_HIP(hipStreamSynchronize(stream_));
        timer_.collect();
    }

    bool all_stopped()
    {
        std::vector<Scal> sc(params_.populations);
        scal_.download(sc.data(), sc.size());
        inspect(sc);
        for (const auto &s : sc)
            if (!s.stop) return false;
        return true;
    }

    // get("profile") / set("profile") with the engine's kernel slots
    int profile_report(double *out, int cap) const { return timer_.report(out, cap); }
    int profile_enable(const double *in, int nslots, const char *const *names)
    {
        timer_.enable(in[0] != 0., nslots, names);
        static const char *const prog_names[1] = { "bbo:prog_eval" };
        prog_timer_.enable(in[0] != 0., 1, prog_names);     // (its own report: "prog_profile")
        return 1;
    }

    bbo_params params_;
    ObjectiveSpec obj_;
    hipStream_t stream_ = nullptr;
    bool inited_ = false;
    KernelTimer timer_;
    ProgEval prog_;             // the objective program's evaluation launches (obj_.is_program())
    KernelTimer prog_timer_;    // their time, outside the engine's own slots
    std::vector<double> lower_h_, upper_h_, aux_h_;
    DevBuf<double> lower_, upper_, aux_;
    DevBuf<Scal> scal_;
};

// the modes of a walk kernel (the engines' own enums name the same values for their kernels)
enum WalkMode {
    WALK_FUSED = 0,          // a whole generation, the evaluations inside
    WALK_ADVANCE,            // up to the next pending evaluation (phase 0)
    WALK_ABSORB              // take the value of the pending evaluation (phase 2)
};

// The engines whose generation is one workgroup's walk per population (SLPSO, CRS, SSDE): with a
// device objective one fused launch, with a host objective the same walk entered and left at its
// evaluations, every round one point per population that still has one pending.  The layer owns that
// loop, the same steps one at a time (phase) and the flag that says a generation is under way.
template<class Scal>
class WalkEngine: public Engine<Scal> {
public:
    // bbo_<engine>_phase: 0 advance to the next pending evaluation, 1 evaluate, 2 absorb
    void phase(int which)
    {
        this->run_phase(phase_fn_, which, 3, std::string(phase_fn_) + ": 0 advance, 1 evaluate, 2 absorb", [&] {
            honor_stop() = 0;
            if (which == 0) {
                // the first advance of a generation starts it in every population; the later ones leave a
                // population that has completed it alone until none has a point pending
                launch_walk(WALK_ADVANCE, !mid_generation_);
                mid_generation_ = any_pending();
            } else if (which == 1) {
                launch_eval();
            } else {
                launch_walk(WALK_ABSORB, false);
                if (absorb_advances_) mid_generation_ = any_pending();
            }
        });
    }

protected:
    // absorb_advances: the kernel's WALK_ABSORB walks on to the next pending point itself (CRS)
    WalkEngine(const bbo_params &p, const char *phase_fn, bool absorb_advances) :
            Engine<Scal>(p), phase_fn_(phase_fn), absorb_advances_(absorb_advances)
    {
    }

    // ---- the hooks ----------------------------------------------------------------------------
    // one launch of the walk in every population (WALK_FUSED: whole, whatever launches that takes);
    // `begin`: an idle population starts its next generation
    virtual void launch_walk(int mode, bool begin) = 0;
    // the device objective at every population's pending point
    virtual void launch_eval_device() = 0;
    virtual PendingPoints pending_points(int p, const Scal &s) = 0;
    // the kernels' copy of the flag: a stopped population takes no further generation
    virtual int &honor_stop() = 0;

    void generation(bool honor) override
    {
        honor_stop() = honor ? 1 : 0;
        if (!this->obj_.needs_host()) {
            launch_walk(WALK_FUSED, true);
        } else {
            launch_walk(WALK_ADVANCE, !mid_generation_);
            while (any_pending()) {
                launch_eval();
                launch_walk(WALK_ABSORB, false);
                if (!absorb_advances_) launch_walk(WALK_ADVANCE, false);
            }
        }
        mid_generation_ = false;
    }

    bool mid_generation_ = false;    // phase(): some population has a point pending

private:
    // the value of every population's pending point
    void launch_eval()
    {
        if (!this->obj_.needs_host()) launch_eval_device();
        else this->host_evaluate_pending(honor_stop() != 0, [this](int p, const Scal &s) { return pending_points(p, s); });
    }

    bool any_pending()
    {
        BBO_HIP(hipStreamSynchronize(this->stream_));
        std::vector<Scal> sc(this->params_.populations);
        this->scal_.download(sc.data(), sc.size());
        for (const auto &s : sc)
            if (s.pending && !(honor_stop() && s.stop)) return true;
        return false;
    }

    const char *phase_fn_;
    const bool absorb_advances_;
};

} // namespace bbo
