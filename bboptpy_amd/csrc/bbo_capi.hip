// bbo_capi.hip -- the extern "C" surface declared in include/bbopt_hip.h.
// Each entry point catches bbo::Error / std::exception and turns it into a status code
// plus a message retrievable with bbo_last_error(), so no C++ exception crosses the ABI.
#include "bbo_cma.hpp"
#include "bbo_ccpso.hpp"
#include "bbo_jaya.hpp"
#include "bbo_dsa.hpp"
#include "bbo_hees.hpp"
#include "bbo_spiral.hpp"
#include "bbo_nshs.hpp"
#include "bbo_lm.hpp"
#include "bbo_xnes.hpp"
#include "bbo_amalgam.hpp"
#include "bbo_slpso.hpp"
#include "bbo_crs.hpp"
#include "bbo_ssde.hpp"
#include "bbo_acd.hpp"
#include "bbo_mayfly.hpp"
#include "bbo_pikaia.hpp"
#include "bbo_nm.hpp"
#include "bbo_rosen.hpp"
#include "bbo_bh.hpp"

#include <cstddef>
#include <memory>
#include <mutex>
#include <set>

namespace bbo {
Optimizer* make_de_engine(const bbo_params &p);       // bbo_de.hip
Optimizer* make_pso_engine(const bbo_params &p);      // bbo_pso.hip
Optimizer* make_cso_engine(const bbo_params &p);      // bbo_cso.hip
Optimizer* make_ccpso_engine(const bbo_params &p);    // bbo_ccpso.hip
Optimizer* make_jaya_engine(const bbo_params &p);     // bbo_jaya.hip
Optimizer* make_dsa_engine(const bbo_params &p);      // bbo_dsa.hip
Optimizer* make_hees_engine(const bbo_params &p);     // bbo_hees.hip
Optimizer* make_spiral_engine(const bbo_params &p);   // bbo_spiral.hip
Optimizer* make_nshs_engine(const bbo_params &p);     // bbo_nshs.hip
Optimizer* make_lm_engine(const bbo_params &p);       // bbo_lm.hip
Optimizer* make_xnes_engine(const bbo_params &p);     // bbo_xnes.hip
Optimizer* make_amalgam_engine(const bbo_params &p);  // bbo_amalgam.hip
Optimizer* make_slpso_engine(const bbo_params &p);    // bbo_slpso.hip
Optimizer* make_crs_engine(const bbo_params &p);      // bbo_crs.hip
Optimizer* make_ssde_engine(const bbo_params &p);     // bbo_ssde.hip
Optimizer* make_acd_engine(const bbo_params &p);      // bbo_acd.hip
Optimizer* make_mayfly_engine(const bbo_params &p);   // bbo_mayfly.hip
Optimizer* make_pikaia_engine(const bbo_params &p);   // bbo_pikaia.hip
Optimizer* make_nm_engine(const bbo_params &p);       // bbo_nm.hip
Optimizer* make_rosen_engine(const bbo_params &p);    // bbo_rosen.hip
Optimizer* make_restart_driver(const bbo_params &p, Optimizer *base);   // bbo_restart.hip
Optimizer* make_bh_engine(const bbo_params &p, Optimizer *minimizer);   // bbo_bh.hip
void probe_objective(int obj, int form, int n, int rows, const double *X, double *f_out);   // bbo_probe.hip
}

// the caller's share of a compiled objective program; handles initialised with it hold their own
struct bbo_program_s {
    std::shared_ptr<bbo::Program> prog;
};

struct bbo_handle_s {
    std::unique_ptr<bbo::Optimizer> opt;
    std::string error;
    int algo = 0;
};

namespace {

std::string g_create_error;
std::mutex g_create_mutex;

// the live bbo_program objects: `user` of a PROGRAM objective is checked against them
std::set<bbo_program> g_programs;
std::mutex g_programs_mutex;

// the tail of every entry point on a handle: `fn` returns the call's int (a count, or BBO_OK)
template<class F>
int guarded_value(bbo_handle h, F fn)
{
    if (!h || !h->opt) return BBO_ERR_ARG;
    try {
        return fn();
    } catch (const bbo::Error &e) {
        h->error = e.what();
        return e.status;
    } catch (const std::exception &e) {
        h->error = e.what();
        return BBO_ERR_HIP;
    }
}

template<class F>
int guarded(bbo_handle h, F fn)
{
    return guarded_value(h, [&] {
        fn();
        return (int) BBO_OK;
    });
}

// the same for the calls that make an object: their message is the one of bbo_last_error(NULL)
template<class F>
int created(const char *fn, bool have_args, F make)
{
    std::lock_guard<std::mutex> lock(g_create_mutex);
    if (!have_args) {
        g_create_error = std::string(fn) + ": NULL argument";
        return BBO_ERR_ARG;
    }
    try {
        make();
        return BBO_OK;
    } catch (const bbo::Error &e) {
        g_create_error = e.what();
        return e.status;
    } catch (const std::exception &e) {
        g_create_error = e.what();
        return BBO_ERR_HIP;
    }
}

// the engine behind a handle as the class an extension entry point needs; T::HANDLE_NAME is its refusal
template<class T>
T *engine_of(bbo_handle h)
{
    auto *e = dynamic_cast<T*>(h->opt.get());
    if (!e) throw bbo::Error(BBO_ERR_ARG, T::HANDLE_NAME);
    return e;
}

// bbo_<engine>_configure
template<class T, class Params>
int configure_of(bbo_handle h, const Params *p, const char *fn)
{
    return guarded(h, [&] {
        if (!p) throw bbo::Error(BBO_ERR_ARG, std::string(fn) + ": NULL parameters");
        engine_of<T>(h)->configure(*p);
    });
}

bbo::Optimizer *make_cma_engine(const bbo_params &p)
{
    return new bbo::CmaEngine(p);
}

// bbo_create: the engine of every algorithm (the restart drivers have bbo_create_restart)
const struct {
    int algo;
    bbo::Optimizer *(*make)(const bbo_params&);
} FACTORIES[] = {
    { BBO_ALGO_CMAES, make_cma_engine }, { BBO_ALGO_ACTIVE_CMAES, make_cma_engine },
    { BBO_ALGO_SEP_CMAES, make_cma_engine }, { BBO_ALGO_CHOLESKY_CMAES, make_cma_engine },
    { BBO_ALGO_SHADE, bbo::make_de_engine }, { BBO_ALGO_JADE, bbo::make_de_engine },
    { BBO_ALGO_SANSDE, bbo::make_de_engine }, { BBO_ALGO_APSO, bbo::make_pso_engine },
    { BBO_ALGO_CSO, bbo::make_cso_engine }, { BBO_ALGO_CCPSO, bbo::make_ccpso_engine },
    { BBO_ALGO_JAYA, bbo::make_jaya_engine }, { BBO_ALGO_DSA, bbo::make_dsa_engine },
    { BBO_ALGO_HEES, bbo::make_hees_engine }, { BBO_ALGO_SPIRAL, bbo::make_spiral_engine },
    { BBO_ALGO_NSHS, bbo::make_nshs_engine }, { BBO_ALGO_LM_CMAES, bbo::make_lm_engine },
    { BBO_ALGO_XNES, bbo::make_xnes_engine }, { BBO_ALGO_AMALGAM, bbo::make_amalgam_engine },
    { BBO_ALGO_SLPSO, bbo::make_slpso_engine }, { BBO_ALGO_CRS, bbo::make_crs_engine },
    { BBO_ALGO_SSDE, bbo::make_ssde_engine }, { BBO_ALGO_ACD, bbo::make_acd_engine },
    { BBO_ALGO_MAYFLY, bbo::make_mayfly_engine }, { BBO_ALGO_PIKAIA, bbo::make_pikaia_engine },
    { BBO_ALGO_NELDER_MEAD, bbo::make_nm_engine }, { BBO_ALGO_ROSENBROCK, bbo::make_rosen_engine },
};

bbo::ObjectiveSpec to_spec(const bbo_objective *o)
{
    if (!o) throw bbo::Error(BBO_ERR_ARG, "objective must not be NULL");
    bbo::ObjectiveSpec s;
    s.kind = o->kind;
    s.builtin = o->builtin;
    s.scalar = o->scalar;
    s.batch = o->batch;
    s.user = o->user;
    if (s.kind == BBO_OBJECTIVE_BUILTIN) {
        if (s.builtin < 0 || s.builtin > BBO_OBJ_SCHWEFEL12)
            throw bbo::Error(BBO_ERR_ARG, "unknown builtin objective id");
    } else if (s.kind == BBO_OBJECTIVE_SCALAR_CALLBACK) {
        if (!s.scalar) throw bbo::Error(BBO_ERR_ARG, "scalar callback is NULL");
    } else if (s.kind == BBO_OBJECTIVE_BATCH_CALLBACK) {
        if (!s.batch) throw bbo::Error(BBO_ERR_ARG, "batch callback is NULL");
    } else if (s.kind == BBO_OBJECTIVE_PROGRAM) {
        std::lock_guard<std::mutex> lock(g_programs_mutex);
        const auto it = g_programs.find(static_cast<bbo_program>(s.user));
        if (it == g_programs.end())
            throw bbo::Error(BBO_ERR_ARG, "objective kind PROGRAM: `user` is not a live bbo_program");
        s.program = (*it)->prog;
    } else {
        throw bbo::Error(BBO_ERR_ARG, "unknown objective kind");
    }
    return s;
}

// bbo_params as a caller built against an earlier header knows it ends where `stol` begins.  Such a
// caller can only name the algorithms of its header, so the fields appended for CholeskyCMAES are
// read and written for BBO_ALGO_CHOLESKY_CMAES, BBO_ALGO_DSA, BBO_ALGO_AMALGAM, BBO_ALGO_SLPSO and BBO_ALGO_ACD (whose
// `stol` travels there: a caller that can name algorithm 13, 19, 20 or 23 has the long struct) alone: nothing here touches memory past
// the struct the caller allocated.
constexpr size_t PARAMS_BASE_BYTES = offsetof(bbo_params, stol);

inline bool has_long_params(int algo)
{
    return algo == BBO_ALGO_CHOLESKY_CMAES || algo == BBO_ALGO_DSA || algo == BBO_ALGO_AMALGAM
            || algo == BBO_ALGO_SLPSO || algo == BBO_ALGO_ACD;
}

bbo_params own_copy(const bbo_params *params)
{
    bbo_params p;
    std::memset(&p, 0, sizeof(p));
    std::memcpy(&p, params, has_long_params(params->algo) ? sizeof(p) : PARAMS_BASE_BYTES);
    return p;
}

} // namespace

#include <dlfcn.h>
namespace bbo {
const Roctx &Roctx::get()
{
    static const Roctx r = [] {
        Roctx x;
        for (const char *lib : { "librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4",
                "libroctx64.so" }) {
            void *h = dlopen(lib, RTLD_LAZY | RTLD_LOCAL);
            if (!h) continue;
            x.push = reinterpret_cast<Roctx::push_fn>(dlsym(h, "roctxRangePushA"));
            x.pop = reinterpret_cast<Roctx::pop_fn>(dlsym(h, "roctxRangePop"));
            if (x.push && x.pop) break;
            x.push = nullptr;
            x.pop = nullptr;
        }
        return x;
    }();
    return r;
}
} // namespace bbo

extern "C" {

void bbo_params_default(bbo_params *p, int algo)
{
    if (!p) return;
    std::memset(p, 0, has_long_params(algo) ? sizeof(*p) : PARAMS_BASE_BYTES);
    p->algo = algo;
    // defaults of py/multivariate_py.cpp:103-171,265-269
    p->sigma0 = 2.;
    p->bound = 0;
    p->alphacov = 2.;
    p->eigenrate = 0.25;
    p->archive = 1;
    p->repaircr = 1;
    p->pelite = 0.05;
    p->cdamp = 0.1;
    p->jade_sigma = 0.07;
    p->h = 100;
    p->npmin = 4;
    p->correct = 1;
    p->print = 0;
    p->nipop = 1;
    p->ksigmadec = 1.6;
    p->boundlambda = 1;
    p->maxlargeruns = 9;
    p->kbudget = 2.;
    p->seed = 0x9E3779B97F4A7C15ull;
    p->device = 0;
    p->populations = 1;
    p->poll_every = 8;
    p->adjustlr = 1;   /* py/multivariate_py.cpp:131-135: "adjustlr"_a = true */
    p->crref = 5;
    p->pupdate = 50;
    p->crupdate = 25;
    p->pcompete = 3;
    p->ring = 0;
    p->vmax = 0.2;
    p->npps = 0;
    p->pcauchy = -1.;
    if (algo == BBO_ALGO_SPIRAL) p->np = 20;   /* py/multivariate_py.cpp:348 */
    if (algo == BBO_ALGO_NSHS || algo == BBO_ALGO_CRS) p->poll_every = 0;   /* the engine's own chunk: iterations, not generations */
    if (algo == BBO_ALGO_ACD) p->poll_every = 0;    /* one sweep of n coordinate steps */
    if (algo == BBO_ALGO_NELDER_MEAD) p->poll_every = 0;    /* the engine's own chunk of simplex steps */
    if (algo == BBO_ALGO_ROSENBROCK) p->poll_every = 0;     /* the engine's own chunk of line searches */
    if (algo == BBO_ALGO_BASIN_HOPPING) p->poll_every = 0;  /* the engine's own count of rounds */
    if (has_long_params(algo)) {               // (see PARAMS_BASE_BYTES)
        p->stol = 0.;
        p->ranked = 0;
    }
}

int bbo_create(const bbo_params *params, bbo_handle *out)
{
    return created("bbo_create", params && out, [&] {
        *out = nullptr;
        std::unique_ptr<bbo_handle_s> h(new bbo_handle_s());
        h->algo = params->algo;
        const bbo_params own = own_copy(params);
        for (const auto &f : FACTORIES)
            if (f.algo == own.algo) {
                h->opt.reset(f.make(own));
                *out = h.release();
                return;
            }
        throw bbo::Error(BBO_ERR_ARG, "bbo_create: unknown algo (restart drivers use bbo_create_restart)");
    });
}

int bbo_create_restart(const bbo_params *params, bbo_handle base, bbo_handle *out)
{
    return created("bbo_create_restart", params && out && base && base->opt, [&] {
        *out = nullptr;
        if (params->algo != BBO_ALGO_IPOP_CMAES && params->algo != BBO_ALGO_BIPOP_CMAES)
            throw bbo::Error(BBO_ERR_ARG, "bbo_create_restart: algo must be IPOP or BIPOP");
        if (base->algo != BBO_ALGO_CMAES && base->algo != BBO_ALGO_ACTIVE_CMAES
                && base->algo != BBO_ALGO_SEP_CMAES && base->algo != BBO_ALGO_CHOLESKY_CMAES)
            throw bbo::Error(BBO_ERR_ARG, "bbo_create_restart: base must be a CMA-ES handle");
        std::unique_ptr<bbo_handle_s> h(new bbo_handle_s());
        h->algo = params->algo;
        const bbo_params own = own_copy(params);
        h->opt.reset(bbo::make_restart_driver(own, base->opt.get()));
        *out = h.release();
    });
}

int bbo_create_basin(const bbo_params *params, bbo_handle minimizer, bbo_handle *out)
{
    return created("bbo_create_basin", params && out && minimizer && minimizer->opt, [&] {
        *out = nullptr;
        if (params->algo != BBO_ALGO_BASIN_HOPPING)
            throw bbo::Error(BBO_ERR_ARG, "bbo_create_basin: algo must be BBO_ALGO_BASIN_HOPPING");
        std::unique_ptr<bbo_handle_s> h(new bbo_handle_s());
        h->algo = params->algo;
        h->opt.reset(bbo::make_bh_engine(own_copy(params), minimizer->opt.get()));
        *out = h.release();
    });
}

int bbo_program_create(const char *source, const char *arch, const double *data, int data_count,
        bbo_program *out)
{
    return created("bbo_program_create", out != nullptr, [&] {
        *out = nullptr;
        std::unique_ptr<bbo_program_s> p(new bbo_program_s());
        p->prog = bbo::Program::compile(source, arch, data, data_count);
        std::lock_guard<std::mutex> reg(g_programs_mutex);
        g_programs.insert(p.get());
        *out = p.release();
    });
}

int bbo_program_destroy(bbo_program p)
{
    if (!p) return BBO_OK;
    {
        std::lock_guard<std::mutex> reg(g_programs_mutex);
        if (!g_programs.erase(p)) return BBO_ERR_ARG;
    }
    delete p;
    return BBO_OK;
}

int bbo_destroy(bbo_handle h)
{
    delete h;
    return BBO_OK;
}

int bbo_init(bbo_handle h, int n, const double *lower, const double *upper,
        const double *guess, const bbo_objective *objective)
{
    return guarded(h, [&] {
        if (!lower || !upper || !guess) throw bbo::Error(BBO_ERR_ARG, "NULL bound/guess");
        h->opt->init(n, lower, upper, guess, to_spec(objective));
    });
}

int bbo_iterate(bbo_handle h)
{
    return guarded(h, [&] { h->opt->iterate(); });
}

int bbo_solution(bbo_handle h, double *x_out, int *n_evals, int *converged)
{
    return bbo_solution_of(h, 0, x_out, n_evals, converged);
}

int bbo_solution_of(bbo_handle h, int population, double *x_out, int *n_evals,
        int *converged)
{
    return guarded(h, [&] {
        if (!x_out || !n_evals || !converged) throw bbo::Error(BBO_ERR_ARG, "NULL output");
        h->opt->solution(population, x_out, n_evals, converged);
    });
}

int bbo_optimize(bbo_handle h, int n, const double *lower, const double *upper,
        const double *guess, const bbo_objective *objective, double *x_out, int *n_evals,
        int *converged)
{
    return guarded(h, [&] {
        if (!lower || !upper || !guess || !x_out || !n_evals || !converged)
            throw bbo::Error(BBO_ERR_ARG, "NULL argument");
        h->opt->optimize(n, lower, upper, guess, to_spec(objective), x_out, n_evals,
                converged);
    });
}

int bbo_run(bbo_handle h, int max_generations, int *generations_done)
{
    return guarded(h, [&] {
        const int g = h->opt->run(max_generations);
        if (generations_done) *generations_done = g;
    });
}

int bbo_get(bbo_handle h, const char *key, int population, double *out, int cap)
{
    if (!key) return BBO_ERR_ARG;
    return guarded_value(h, [&] { return h->opt->get(key, population, out, cap); });
}

int bbo_set(bbo_handle h, const char *key, int population, const double *in, int count)
{
    if (!key || !in) return BBO_ERR_ARG;
    return guarded_value(h, [&] { return h->opt->set(key, population, in, count); });
}

int bbo_cma_phase_run(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::CmaEngine>(h)->phase(phase); });
}

int bbo_cma_inject_normals(bbo_handle h, const double *z, int count)
{
    return guarded(h, [&] { engine_of<bbo::CmaEngine>(h)->inject_normals(z, count); });
}

int bbo_cma_set_params(bbo_handle h, int np, double sigma0, int mfev)
{
    return guarded(h, [&] {
        auto *cma = engine_of<bbo::CmaEngine>(h);
        if (np < 4) throw bbo::Error(BBO_ERR_ARG, "CMA-ES needs np >= 4");
        cma->set_params(np, sigma0, mfev);
    });
}

int bbo_cma_set_seed(bbo_handle h, uint64_t seed)
{
    return guarded(h, [&] { engine_of<bbo::CmaEngine>(h)->set_seed(seed); });
}

int bbo_cma_evaluate(bbo_handle h, const double *x, double *f_out)
{
    return guarded(h, [&] {
        auto *cma = engine_of<bbo::CmaEngine>(h);
        if (!x || !f_out) throw bbo::Error(BBO_ERR_ARG, "NULL argument");
        if (cma->dimension() <= 0) throw bbo::Error(BBO_ERR_STATE, "evaluate before initialize()");
        *f_out = cma->evaluate_point(x);
    });
}

int bbo_ccpso_set_shard(bbo_handle h, int rank, int world)
{
    return guarded(h, [&] { engine_of<bbo::CcpsoEngine>(h)->set_shard(rank, world); });
}

int bbo_ccpso_set_local(bbo_handle h, bbo_handle local, int localfreq)
{
    return guarded(h, [&] {
        if (local && !local->opt) throw bbo::Error(BBO_ERR_ARG, "bbo_ccpso_set_local: dead local handle");
        if (local == h) throw bbo::Error(BBO_ERR_ARG, "bbo_ccpso_set_local: local must be another optimizer");
        engine_of<bbo::CcpsoEngine>(h)->set_local(local ? local->opt.get() : nullptr, localfreq);
    });
}

int bbo_ccpso_phase(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::CcpsoEngine>(h)->phase(phase); });
}

int bbo_ccpso_table_record(bbo_handle h)
{
    return guarded_value(h, [&] { return engine_of<bbo::CcpsoEngine>(h)->table_record(); });
}

int bbo_ccpso_export_tables(bbo_handle h, double *dst, int device_memory)
{
    return guarded(h, [&] {
        if (!dst) throw bbo::Error(BBO_ERR_ARG, "NULL destination");
        engine_of<bbo::CcpsoEngine>(h)->export_tables(dst, device_memory != 0);
    });
}

int bbo_ccpso_merge_tables(bbo_handle h, const double *gathered, int world, int device_memory)
{
    return guarded(h, [&] {
        if (!gathered) throw bbo::Error(BBO_ERR_ARG, "NULL source");
        engine_of<bbo::CcpsoEngine>(h)->merge_tables(gathered, world, device_memory != 0);
    });
}

void bbo_jaya_params_default(bbo_jaya_params *p)
{
    if (!p) return;
    // defaults of py/multivariate_py.cpp:226-234
    p->adapt = 1;
    p->k0 = 2;
    p->mutation = BBO_JAYA_LOGISTIC;
    p->kcheb = 2;
    p->scale = 0.01;
    p->beta = 1.5;
    p->temper = 10.;
}

int bbo_jaya_configure(bbo_handle h, const bbo_jaya_params *p)
{
    return configure_of<bbo::JayaEngine>(h, p, "bbo_jaya_configure");
}

void bbo_dsa_params_default(bbo_dsa_params *p)
{
    if (!p) return;
    // defaults of py/multivariate_py.cpp:189-191
    p->adapt = 1;
    p->nbatch = 100;
}

int bbo_dsa_configure(bbo_handle h, const bbo_dsa_params *p)
{
    return configure_of<bbo::DsaEngine>(h, p, "bbo_dsa_configure");
}

void bbo_hees_params_default(bbo_hees_params *p)
{
    if (!p) return;
    // defaults of py/multivariate_py.cpp:206-211
    p->mres = 1;
    p->print = 0;
}

int bbo_hees_configure(bbo_handle h, const bbo_hees_params *p)
{
    return configure_of<bbo::HeesEngine>(h, p, "bbo_hees_configure");
}

int bbo_hees_phase(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::HeesEngine>(h)->phase(phase); });
}

int bbo_hees_inject_normals(bbo_handle h, const double *z, int count)
{
    return guarded(h, [&] { engine_of<bbo::HeesEngine>(h)->inject_normals(z, count); });
}

void bbo_spiral_params_default(bbo_spiral_params *p)
{
    if (!p) return;
    // defaults of py/multivariate_py.cpp:348-350, as printed there
    p->r = 0.95;
    p->theta = 1.57079632679;
    p->taur = 0.;
    p->tautheta = 0.1;
    p->rlow = 0.9;
    p->rhigh = 1.;
    p->thetalow = 0.;
    p->thetahigh = 6.28318530718;
}

int bbo_spiral_configure(bbo_handle h, const bbo_spiral_params *p)
{
    return configure_of<bbo::SpiralEngine>(h, p, "bbo_spiral_configure");
}

int bbo_spiral_phase(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::SpiralEngine>(h)->phase(phase); });
}

int bbo_spiral_inject_uniforms(bbo_handle h, const double *u, int count)
{
    return guarded(h, [&] { engine_of<bbo::SpiralEngine>(h)->inject_uniforms(u, count); });
}

void bbo_nshs_params_default(bbo_nshs_params *p)
{
    if (!p) return;
    p->fstdmin = 0.0001;        // py/multivariate_py.cpp:204
}

int bbo_nshs_configure(bbo_handle h, const bbo_nshs_params *p)
{
    return configure_of<bbo::NshsEngine>(h, p, "bbo_nshs_configure");
}

int bbo_nshs_phase(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::NshsEngine>(h)->phase(phase); });
}

int bbo_nshs_inject_uniforms(bbo_handle h, const double *u, int count)
{
    return guarded(h, [&] { engine_of<bbo::NshsEngine>(h)->inject_uniforms(u, count); });
}

void bbo_lm_params_default(bbo_lm_params *p)
{
    if (!p) return;
    // defaults of py/multivariate_py.cpp:126-127
    p->memory = 0;
    p->rademacher = 1;
    p->usenew = 1;
}

int bbo_lm_configure(bbo_handle h, const bbo_lm_params *p)
{
    return configure_of<bbo::LmEngine>(h, p, "bbo_lm_configure");
}

int bbo_lm_phase(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::LmEngine>(h)->phase(phase); });
}

int bbo_lm_inject_draws(bbo_handle h, const double *table, int count)
{
    return guarded(h, [&] { engine_of<bbo::LmEngine>(h)->inject_draws(table, count); });
}

void bbo_xnes_params_default(bbo_xnes_params *p)
{
    if (!p) return;
    // defaults of py/multivariate_py.cpp (xNES: a0 = 1., etamu = 1.); from_guess is an extension
    p->a0 = 1.;
    p->etamu = 1.;
    p->from_guess = 0;
}

int bbo_xnes_configure(bbo_handle h, const bbo_xnes_params *p)
{
    return configure_of<bbo::XnesEngine>(h, p, "bbo_xnes_configure");
}

int bbo_xnes_phase(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::XnesEngine>(h)->phase(phase); });
}

int bbo_xnes_inject_normals(bbo_handle h, const double *z, int count)
{
    return guarded(h, [&] { engine_of<bbo::XnesEngine>(h)->inject_normals(z, count); });
}

void bbo_amalgam_params_default(bbo_amalgam_params *p)
{
    if (!p) return;
    // defaults of py/multivariate_py.cpp (AMALGAM: iamalgam, noparam, print = true); the rest are extensions
    p->iamalgam = 1;
    p->noparam = 1;
    p->print = 1;
    p->keep_elite = 0;
    p->concurrent = 1;
    p->substream = 0;
}

int bbo_amalgam_configure(bbo_handle h, const bbo_amalgam_params *p)
{
    return configure_of<bbo::AmalgamEngine>(h, p, "bbo_amalgam_configure");
}

int bbo_amalgam_phase(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::AmalgamEngine>(h)->phase(phase); });
}

int bbo_amalgam_inject_draws(bbo_handle h, const double *z, int zcount, const int *rows, int rcount)
{
    return guarded(h, [&] { engine_of<bbo::AmalgamEngine>(h)->inject_draws(z, zcount, rows, rcount); });
}

int bbo_amalgam_inject_points(bbo_handle h, const double *x, int count)
{
    return guarded(h, [&] { engine_of<bbo::AmalgamEngine>(h)->inject_points(x, count); });
}

void bbo_slpso_params_default(bbo_slpso_params *p)
{
    if (!p) return;
    // py/multivariate_py.cpp:292-299
    p->omegamin = 0.4;
    p->omegamax = 0.9;
    p->eta = 1.496;
    p->gamma = 0.01;
    p->vmax = 0.2;
    p->Ufmax = 10.;
}

int bbo_slpso_configure(bbo_handle h, const bbo_slpso_params *p)
{
    return configure_of<bbo::SlpsoEngine>(h, p, "bbo_slpso_configure");
}

int bbo_slpso_phase(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::SlpsoEngine>(h)->phase(phase); });
}

int bbo_slpso_inject_draws(bbo_handle h, const double *table, int count)
{
    return guarded(h, [&] { engine_of<bbo::SlpsoEngine>(h)->inject_draws(table, count); });
}

void bbo_crs_params_default(bbo_crs_params *p)
{
    if (!p) return;
    p->max_depth = 4096;
    p->repair = 0;
}

int bbo_crs_configure(bbo_handle h, const bbo_crs_params *p)
{
    return configure_of<bbo::CrsEngine>(h, p, "bbo_crs_configure");
}

int bbo_crs_phase(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::CrsEngine>(h)->phase(phase); });
}

int bbo_crs_inject_draws(bbo_handle h, const double *table, int count)
{
    return guarded(h, [&] { engine_of<bbo::CrsEngine>(h)->inject_draws(table, count); });
}

void bbo_ssde_params_default(bbo_ssde_params *p)
{
    if (!p) return;
    /* the Python binding's defaults (py/multivariate_py.cpp): its usede is false, the C++ header's true */
    p->patience = 1000;
    p->npmin = 4;
    p->ptop = 0.11;
    p->h = 100;
    p->usede = 0;
    p->repaircr = 1;
}

int bbo_ssde_configure(bbo_handle h, const bbo_ssde_params *p)
{
    return configure_of<bbo::SsdeEngine>(h, p, "bbo_ssde_configure");
}

int bbo_ssde_phase(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::SsdeEngine>(h)->phase(phase); });
}

int bbo_ssde_inject_draws(bbo_handle h, const double *table, int count)
{
    return guarded(h, [&] { engine_of<bbo::SsdeEngine>(h)->inject_draws(table, count); });
}

void bbo_acd_params_default(bbo_acd_params *p)
{
    if (!p) return;
    p->ksucc = 2.;      /* py/multivariate_py.cpp:44-48 */
    p->kunsucc = 0.5;
    p->from_guess = 0;
    p->speculate = 0;
}

int bbo_acd_configure(bbo_handle h, const bbo_acd_params *p)
{
    return configure_of<bbo::AcdEngine>(h, p, "bbo_acd_configure");
}

int bbo_acd_phase(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::AcdEngine>(h)->phase(phase); });
}

void bbo_mayfly_params_default(bbo_mayfly_params *p)
{
    if (!p) return;
    /* py/multivariate_py.cpp:236-246 (commented away there), mayfly.h:64-68 */
    p->a1 = 1.;
    p->a2 = 1.5;
    p->a3 = 1.5;
    p->beta = 2.;
    p->dance = 5.;
    p->ddamp = 0.8;
    p->fl = 1.;
    p->fldamp = 0.99;
    p->gmin = 0.8;
    p->gmax = 0.8;
    p->vdamp = 0.1;
    p->sigma = 0.1;
    p->pmutdim = 0.01;
    p->pmutnp = 0.05;
    p->l = 0.95;
    p->pgb = 0;
    p->repair = 0;
    p->substream = 0;
}

int bbo_mayfly_configure(bbo_handle h, const bbo_mayfly_params *p)
{
    return configure_of<bbo::MayflyEngine>(h, p, "bbo_mayfly_configure");
}

int bbo_mayfly_inject_draws(bbo_handle h, const double *table, int count)
{
    return guarded(h, [&] { engine_of<bbo::MayflyEngine>(h)->inject_draws(table, count); });
}

void bbo_pikaia_params_default(bbo_pikaia_params *p)
{
    if (!p) return;
    /* pikaia.h:25-27 */
    p->pcross = 0.85;
    p->pmut = 0.005;
    p->pmutmn = 0.0005;
    p->pmutmx = 0.25;
    p->fdif = 1.;
    p->imut = 2;
    p->irep = 1;
    p->ielite = 0;
    p->repair = 0;
    p->raw = 0;
    p->substream = 0;
}

int bbo_pikaia_configure(bbo_handle h, const bbo_pikaia_params *p)
{
    return configure_of<bbo::PikaiaEngine>(h, p, "bbo_pikaia_configure");
}

int bbo_pikaia_inject_draws(bbo_handle h, const double *table, int count)
{
    return guarded(h, [&] { engine_of<bbo::PikaiaEngine>(h)->inject_draws(table, count); });
}

void bbo_nm_params_default(bbo_nm_params *p)
{
    if (!p) return;
    p->minit = 1;       /* py/multivariate_py.cpp:307-337: spendley, mehta2019_refined */
    p->pinit = 3;
    p->checkev = 10;
    p->eps = 1e-3;
    p->repair = 0;
    p->speculate = 0;
    p->lds = -1;
    p->substream = 0;
}

int bbo_nm_configure(bbo_handle h, const bbo_nm_params *p)
{
    return configure_of<bbo::NmEngine>(h, p, "bbo_nm_configure");
}

int bbo_nm_phase(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::NmEngine>(h)->phase(phase); });
}

void bbo_rosen_params_default(bbo_rosen_params *p)
{
    if (!p) return;
    p->decf = 0.1;      /* rosenbrock.h:55 */
    p->repair = 0;
    p->wide = -1;
    p->substream = 0;
}

int bbo_rosen_configure(bbo_handle h, const bbo_rosen_params *p)
{
    return configure_of<bbo::RosenEngine>(h, p, "bbo_rosen_configure");
}

int bbo_rosen_phase(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::RosenEngine>(h)->phase(phase); });
}

void bbo_bh_params_default(bbo_bh_params *p)
{
    if (!p) return;
    /* py/multivariate_py.cpp:83-97: the adaptive strategy's and BasinHopping's defaults */
    p->stepsize = 1.;
    p->adaptive = 1;
    p->accept_rate = 0.5;
    p->interval = 5;
    p->factor = 0.9;
    p->temp = 1.;
    p->mit = 99;
    p->print = 1;
    p->lockstep = -1;
    p->substream = 0;
    p->nstep0 = 0;
    p->naccept0 = 0;
}

int bbo_bh_configure(bbo_handle h, const bbo_bh_params *p)
{
    return configure_of<bbo::BhEngine>(h, p, "bbo_bh_configure");
}

int bbo_bh_phase(bbo_handle h, int phase)
{
    return guarded(h, [&] { engine_of<bbo::BhEngine>(h)->phase(phase); });
}

int bbo_bh_inject_draws(bbo_handle h, const double *table, int count)
{
    return guarded(h, [&] { engine_of<bbo::BhEngine>(h)->inject_draws(table, count); });
}

int bbo_bh_draws(uint64_t seed, int substream, int hop, int n, double *out)
{
    return created("bbo_bh_draws", out != nullptr, [&] {
        if (n < 1 || n > bbo::BH_MAX_N || hop < 0 || substream < 0 || substream >= (1 << 24))
            throw bbo::Error(BBO_ERR_ARG, "bbo_bh_draws: n in [1, 128], hop >= 0, substream in [0, 2^24)");
        bbo::bh_draws_host(seed, substream, hop, n, out);
    });
}

// diagnostics: no handle, so the message is the one of bbo_last_error(NULL)
int bbo_probe_objective(int objective, int form, int n, int rows, const double *X, double *f_out)
{
    return created("bbo_probe_objective", X && f_out,
            [&] { bbo::probe_objective(objective, form, n, rows, X, f_out); });
}

const char* bbo_last_error(bbo_handle h)
{
    if (!h) return g_create_error.c_str();
    return h->error.c_str();
}

const char* bbo_version(void)
{
    return "bbopt_hip 0.1 (gfx950)";
}

int bbo_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

} // extern "C"
