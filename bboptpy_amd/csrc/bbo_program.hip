// bbo_program.hip -- objective programs (bbo_program.hpp): the text of the evaluation kernels that is
// compiled around the user's function, the run-time compiler behind dlopen, the per-device modules,
// and the launches an engine makes.
#include "bbo_common.hpp"
#include "bbo_program.hpp"

#include <hip/hiprtc.h>      // (types and prototypes only: the library is opened at run time)

#include <dlfcn.h>

#include <algorithm>
#include <cstdlib>

namespace bbo {

namespace {

// ---- the translation unit: PRELUDE + the user's source + WRAPPERS -------------------------------
// The wrappers know the user's text by the one function only.  `#line 1` makes the compiler's log
// speak of the user's own lines and columns.
const char PROG_PRELUDE[] =
        "extern \"C\" __device__ double bbo_user_objective(const double *x, int n, const double *data);\n"
        "#line 1 \"objective.hip\"\n";

const char PROG_WRAPPERS[] = R"BBO(
#line 1 "bbo_program_wrappers.hip"
namespace bbo_prog {
struct Plan { const double *X; double *f; int rows; int ld; };
// (the table's pointers are device memory: said so, the loads through them are global loads that
// the compiler may keep in flight across LDS stores, not flat ones)
typedef const __attribute__((address_space(1))) double *gptr;
typedef __attribute__((address_space(1))) double *gptr_w;
__device__ inline double nan_last(double v) { return v != v ? __builtin_huge_val() : v; }
__device__ inline bool stopped(const void *stop, int stride, int p)
{
    return stop && *(const int*) ((const char*) stop + (size_t) p * stride) != 0;
}
}

// Direct form: one lane per candidate, the function reads the row in global memory.
// grid (ceil(max rows / 64), populations), 64 threads.
extern "C" __global__ void __launch_bounds__(64) bbo_prog_eval_direct(const bbo_prog::Plan *plan, int n,
        const double *data, const void *stop, int stop_stride)
{
    const int p = blockIdx.y;
    const bbo_prog::Plan pl = plan[p];
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= pl.rows || bbo_prog::stopped(stop, stop_stride, p)) return;
    const bbo_prog::gptr x = (bbo_prog::gptr) (pl.X + (size_t) row * pl.ld);
    ((bbo_prog::gptr_w) pl.f)[row] = bbo_prog::nan_last(bbo_user_objective((const double*) x, n, data));
}

// Staged form: the wavefront copies its 64 rows (one contiguous block of the population: rows are
// ld doubles apart) into LDS with coalesced loads, row stride `stride` doubles (odd: lanes reading
// coordinate j of 64 different rows fall into different banks), then every lane calls the function
// on its LDS row.  grid as above, 64 threads, dynamic LDS 64 * stride doubles.
extern "C" __global__ void __launch_bounds__(64) bbo_prog_eval_staged(const bbo_prog::Plan *plan, int n,
        const double *data, const void *stop, int stop_stride, int stride)
{
    extern __shared__ double bbo_rows[];
    const int p = blockIdx.y;
    const bbo_prog::Plan pl = plan[p];
    const int row0 = blockIdx.x * 64, lane = threadIdx.x;
    if (row0 >= pl.rows || bbo_prog::stopped(stop, stop_stride, p)) return;     // (uniform)
    const int cnt = min(64, pl.rows - row0);
    const int ld = pl.ld, total = cnt * ld;
    const bbo_prog::gptr src = (bbo_prog::gptr) (pl.X + (size_t) row0 * ld);
    int r = lane / ld, j = lane - r * ld;
#pragma unroll 4
    for (int idx = lane; idx < total; idx += 64) {
        const double v = src[idx];
        if (j < n) bbo_rows[r * stride + j] = v;
        j += 64;
        while (j >= ld) {
            j -= ld;
            r++;
        }
    }
    __syncthreads();
    if (lane < cnt)
        ((bbo_prog::gptr_w) pl.f)[row0 + lane] =
                bbo_prog::nan_last(bbo_user_objective(bbo_rows + lane * stride, n, data));
}
)BBO";

// ---- hiprtc behind dlopen -------------------------------------------------------------------------
struct Rtc {
    decltype(&hiprtcCreateProgram) create = nullptr;
    decltype(&hiprtcCompileProgram) compile = nullptr;
    decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
    decltype(&hiprtcGetProgramLog) log = nullptr;
    decltype(&hiprtcGetCodeSize) code_size = nullptr;
    decltype(&hiprtcGetCode) code = nullptr;
    decltype(&hiprtcDestroyProgram) destroy = nullptr;
    std::string why;        // why it could not be opened
    bool ok = false;

    static const Rtc &get()
    {
        static const Rtc r = [] {
            Rtc x;
            std::vector<std::string> names;
            // (BBO_HIPRTC_LIB: another build of the compiler -- or none, to see the library without it)
            if (const char *e = std::getenv("BBO_HIPRTC_LIB")) names.push_back(e);
            else names = { "libhiprtc.so", "libhiprtc.so.7", "libhiprtc.so.6", "libhiprtc.so.5" };
            void *h = nullptr;
            for (const auto &nm : names) {
                h = dlopen(nm.c_str(), RTLD_LAZY | RTLD_LOCAL);
                if (h) break;
                const char *err = dlerror();
                x.why += (x.why.empty() ? "" : "; ") + std::string(err ? err : nm.c_str());
            }
            if (!h) return x;
#define BBO_RTC_SYM(field, name) x.field = reinterpret_cast<decltype(x.field)>(dlsym(h, name))
            BBO_RTC_SYM(create, "hiprtcCreateProgram");
            BBO_RTC_SYM(compile, "hiprtcCompileProgram");
            BBO_RTC_SYM(log_size, "hiprtcGetProgramLogSize");
            BBO_RTC_SYM(log, "hiprtcGetProgramLog");
            BBO_RTC_SYM(code_size, "hiprtcGetCodeSize");
            BBO_RTC_SYM(code, "hiprtcGetCode");
            BBO_RTC_SYM(destroy, "hiprtcDestroyProgram");
#undef BBO_RTC_SYM
            x.ok = x.create && x.compile && x.log_size && x.log && x.code_size && x.code && x.destroy;
            if (!x.ok) x.why = "the library lacks the hiprtc entry points";
            return x;
        }();
        return r;
    }
};

// the plan of an engine whose populations live in a double buffer, from its device-side scalars
__global__ void prog_fill_plan(ProgPlan *plan, int npop, ProgScalView sv, double *X0, double *X1, double *f0,
        double *f1, int pop_rows, int ld, int which, int rows, int honor_stop)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npop) return;
    const char *rec = (const char*) sv.base + (size_t) p * sv.stride;
    const int cur = *(const int*) (rec + sv.off_cur);
    const int np = *(const int*) (rec + sv.off_np);
    const int stop = *(const int*) (rec + sv.off_stop);
    const int buf = which < 0 ? (cur ^ 1) : which;
    ProgPlan e;
    e.X = (buf == 0 ? X0 : X1) + (size_t) p * pop_rows * ld;
    e.f = (buf == 0 ? f0 : f1) + (size_t) p * pop_rows;
    e.rows = (honor_stop && stop) ? 0 : min(rows, np);
    e.ld = ld;
    plan[p] = e;
}

} // namespace

// ---- Program -----------------------------------------------------------------------------------------
std::shared_ptr<Program> Program::compile(const char *source, const char *arch, const double *data,
        int data_count)
{
    BBO_REQUIRE(source != nullptr, "bbo_program_create: source is NULL");
    BBO_REQUIRE(data_count >= 0 && (data_count == 0 || data != nullptr), "bbo_program_create: bad data table");
    const Rtc &rtc = Rtc::get();
    if (!rtc.ok)
        throw Error(BBO_ERR_ARG, "bbo_program_create: the run-time compiler hiprtc is not available on this "
                "machine (" + rtc.why + "); built-in objectives and host callbacks work without it");
    std::shared_ptr<Program> prog(new Program());
    if (arch) prog->arch_ = arch;
    else {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            throw Error(BBO_ERR_NO_DEVICE, "bbo_program_create: arch is NULL and no HIP device is visible");
        hipDeviceProp_t prop;
        BBO_HIP(hipGetDeviceProperties(&prop, 0));
        prog->arch_ = prop.gcnArchName;
    }
    BBO_REQUIRE(!prog->arch_.empty(), "bbo_program_create: empty architecture string");
    BBO_REQUIRE(prog->arch_.find("xnack+") == std::string::npos,
            "bbo_program_create: xnack+ code objects are not built");
    if (data_count > 0) prog->data_.assign(data, data + data_count);

    // (a text that never names the function cannot define it: say so before the linker does)
    if (std::string(source).find("bbo_user_objective") == std::string::npos)
        throw Error(BBO_ERR_ARG, "objective program: the source does not define bbo_user_objective "
                "(extern \"C\" __device__ double bbo_user_objective(const double *x, int n, const double *data))");

    const std::string unit = std::string(PROG_PRELUDE) + source + "\n" + PROG_WRAPPERS;
    hiprtcProgram rp = nullptr;
    if (rtc.create(&rp, unit.c_str(), "bbo_objective_program.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
        throw Error(BBO_ERR_ARG, "objective program: hiprtcCreateProgram failed");
    // the library's own rule (csrc/Makefile): no contraction, so a program written in the op order of a
    // host function returns the same bits
    const std::string archopt = "--offload-arch=" + prog->arch_;
    const char *opts[] = { archopt.c_str(), "-O3", "-ffp-contract=off", "-std=c++17" };
    const hiprtcResult res = rtc.compile(rp, 4, opts);
    std::string log;
    size_t lsz = 0;
    if (rtc.log_size(rp, &lsz) == HIPRTC_SUCCESS && lsz > 1) {
        log.resize(lsz);
        if (rtc.log(rp, &log[0]) != HIPRTC_SUCCESS) log.clear();
        while (!log.empty() && (log.back() == '\0' || log.back() == '\n')) log.pop_back();
    }
    if (res != HIPRTC_SUCCESS) {
        rtc.destroy(&rp);
        const bool undefined = log.find("bbo_user_objective") != std::string::npos
                && log.find("undefined") != std::string::npos;
        throw Error(BBO_ERR_ARG, std::string(undefined ? "objective program: the source does not define bbo_user_objective"
                                                       : "objective program does not compile")
                + " (" + prog->arch_ + "):\n" + (log.empty() ? "(the compiler left no log)" : log));
    }
    size_t csz = 0;
    if (rtc.code_size(rp, &csz) != HIPRTC_SUCCESS || csz == 0) {
        rtc.destroy(&rp);
        throw Error(BBO_ERR_ARG, "objective program: the compiler returned no code object");
    }
    prog->code_.resize(csz);
    const hiprtcResult cres = rtc.code(rp, prog->code_.data());
    rtc.destroy(&rp);
    if (cres != HIPRTC_SUCCESS) throw Error(BBO_ERR_ARG, "objective program: hiprtcGetCode failed");
    return prog;
}

Program::~Program()
{
    int back = -1;
    if (!loaded_.empty()) (void) hipGetDevice(&back);
    for (auto &kv : loaded_) {
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        if (kv.second.data) (void) hipFree(kv.second.data);
        if (kv.second.module) (void) hipModuleUnload(kv.second.module);
    }
    if (back >= 0) (void) hipSetDevice(back);
}

const Program::Loaded &Program::on_device(int device)
{
    std::lock_guard<std::mutex> lock(mu_);
    auto it = loaded_.find(device);
    if (it != loaded_.end()) return it->second;
    Loaded l;
    const hipError_t e = hipModuleLoadData(&l.module, code_.data());
    if (e != hipSuccess)
        throw Error(BBO_ERR_HIP, "objective program (compiled for " + arch_ + ") does not load on device "
                + std::to_string(device) + ": " + hipGetErrorString(e));
    try {
        BBO_HIP(hipModuleGetFunction(&l.direct, l.module, "bbo_prog_eval_direct"));
        BBO_HIP(hipModuleGetFunction(&l.staged, l.module, "bbo_prog_eval_staged"));
        // (the staged rows of n >= 128 pass 64 KiB a workgroup; where the runtime wants to be told)
        (void) hipFuncSetAttribute((const void*) l.staged, hipFuncAttributeMaxDynamicSharedMemorySize,
                (int) PROG_LDS_PER_CU);
        (void) hipGetLastError();
        const size_t cnt = std::max<size_t>(1, data_.size());
        BBO_HIP(hipMalloc((void**) &l.data, cnt * sizeof(double)));
        BBO_HIP(hipMemset(l.data, 0, cnt * sizeof(double)));
        if (!data_.empty())
            BBO_HIP(hipMemcpy(l.data, data_.data(), data_.size() * sizeof(double), hipMemcpyHostToDevice));
    } catch (...) {
        if (l.data) (void) hipFree(l.data);
        (void) hipModuleUnload(l.module);
        throw;
    }
    return loaded_.emplace(device, l).first->second;
}

// ---- ProgEval ------------------------------------------------------------------------------------------
ProgEval::~ProgEval()
{
    unbind();
}

void ProgEval::unbind()
{
    if (plan_) (void) hipFree(plan_);
    if (xpoint_) (void) hipFree(xpoint_);
    plan_ = nullptr;
    xpoint_ = nullptr;
    prog_.reset();
}

void ProgEval::bind(const std::shared_ptr<Program> &prog, int device, int n, int npop)
{
    unbind();
    BBO_REQUIRE(prog != nullptr, "objective program is NULL");
    fn_ = prog->on_device(device);
    prog_ = prog;
    n_ = n;
    npop_ = npop;
    BBO_HIP(hipMalloc((void**) &plan_, (size_t) (npop + 1) * sizeof(ProgPlan)));
    BBO_HIP(hipMemset(plan_, 0, (size_t) (npop + 1) * sizeof(ProgPlan)));
    BBO_HIP(hipMalloc((void**) &xpoint_, (size_t) (n + 1) * sizeof(double)));
    const ProgPlan one { xpoint_, xpoint_ + n, 1, n };
    BBO_HIP(hipMemcpy(plan_ + npop, &one, sizeof(one), hipMemcpyHostToDevice));
}

void ProgEval::upload_plan(const std::vector<ProgPlan> &plan)
{
    BBO_REQUIRE(bound() && (int) plan.size() == npop_, "objective program: plan size");
    BBO_HIP(hipMemcpy(plan_, plan.data(), plan.size() * sizeof(ProgPlan), hipMemcpyHostToDevice));
}

void ProgEval::fill_plan(hipStream_t st, const ProgScalView &sv, double *X0, double *X1, double *f0,
        double *f1, int pop_rows, int ld, int which, int rows, int honor_stop)
{
    hipLaunchKernelGGL(prog_fill_plan, dim3((npop_ + 63) / 64), dim3(64), 0, st, plan_, npop_, sv, X0, X1, f0, f1,
            pop_rows, ld, which, rows, honor_stop);
    BBO_HIP(hipGetLastError());
}

bool ProgEval::staged() const
{
    if (stage_ >= 0) return stage_ != 0;
    // while the staged rows leave two workgroups to a compute unit (and see PROG_STAGE_MAX_N)
    return n_ <= PROG_STAGE_MAX_N && 2 * prog_stage_bytes(n_) <= PROG_LDS_PER_CU;
}

void ProgEval::launch(hipStream_t st, int max_rows, const void *stop, int stop_stride, KernelTimer *timer)
{
    if (max_rows <= 0) return;
    const ProgPlan *plan = plan_;
    int n = n_;
    const double *data = fn_.data;
    int stride = prog_row_stride(n_);
    const unsigned gx = (unsigned) ((max_rows + PROG_WAVE_ROWS - 1) / PROG_WAVE_ROWS);
    if (timer) timer->begin(st, 0);
    if (staged()) {
        BBO_REQUIRE(prog_stage_bytes(n_) <= PROG_LDS_PER_CU, "prog_stage 1: 64 rows of this dimension do not fit LDS");
        void *args[] = { &plan, &n, &data, &stop, &stop_stride, &stride };
        BBO_HIP(hipModuleLaunchKernel(fn_.staged, gx, (unsigned) npop_, 1, PROG_WAVE_ROWS, 1, 1,
                (unsigned) prog_stage_bytes(n_), st, args, nullptr));
    } else {
        void *args[] = { &plan, &n, &data, &stop, &stop_stride };
        BBO_HIP(hipModuleLaunchKernel(fn_.direct, gx, (unsigned) npop_, 1, PROG_WAVE_ROWS, 1, 1, 0, st, args,
                nullptr));
    }
    if (timer) timer->end(st);
}

// the one-row entry: x up, one lane, the value down
double ProgEval::evaluate_point(hipStream_t st, const double *x)
{
    BBO_REQUIRE(bound(), "objective program is not bound");
    BBO_HIP(hipMemcpyAsync(xpoint_, x, (size_t) n_ * sizeof(double), hipMemcpyHostToDevice, st));
    const ProgPlan *plan = plan_ + npop_;
    int n = n_, stop_stride = 0;
    const double *data = fn_.data;
    const void *stop = nullptr;
    void *args[] = { &plan, &n, &data, &stop, &stop_stride };
    BBO_HIP(hipModuleLaunchKernel(fn_.direct, 1, 1, 1, PROG_WAVE_ROWS, 1, 1, 0, st, args, nullptr));
    double f = 0.;
    BBO_HIP(hipMemcpyAsync(&f, xpoint_ + n_, sizeof(double), hipMemcpyDeviceToHost, st));
    BBO_HIP(hipStreamSynchronize(st));
    return f;
}

} // namespace bbo
