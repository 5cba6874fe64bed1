// bbo_program.hpp -- objective programs: a user's objective as HIP source for one device function,
//     extern "C" __device__ double bbo_user_objective(const double *x, int n, const double *data);
// compiled at run time (hiprtc, opened with dlopen at the first use: the library links against
// nothing it may not find) and evaluated on whole populations on the engine's stream: X and f stay
// in HBM, the host is not waited for.  The compiled unit is prelude + user source + wrapper
// kernels (bbo_program.hip holds their text); DESIGN.md section 3.1.
#pragma once

#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace bbo {

class KernelTimer;

// one population's share of an evaluation launch (grid.y = the entry); rows == 0: nothing to do
struct ProgPlan {
    const double *X;      // rows of ld doubles
    double *f;
    int rows;
    int ld;
};

// Where the plan-filling kernel finds a population's device-side scalars (DE: which half of the
// double buffer holds the trials, how many individuals are alive, the stop flag), as byte offsets
// into the engine's scalar records: the host never reads them back.
struct ProgScalView {
    const void *base;
    int stride;
    int off_cur, off_np, off_stop;
};

// A compiled objective program: the code object for one architecture and the caller's data table.
// Loaded lazily, once per device (the HIP module API), so one program serves handles on several GPUs.
class Program {
public:
    // throws Error(BBO_ERR_ARG, compiler log) when the source does not compile or does not define
    // bbo_user_objective, or when hiprtc cannot be opened.  arch == nullptr: what device 0 reports.
    static std::shared_ptr<Program> compile(const char *source, const char *arch, const double *data,
            int data_count);
    ~Program();

    struct Loaded {
        hipModule_t module = nullptr;
        hipFunction_t direct = nullptr, staged = nullptr;
        double *data = nullptr;
    };
    const Loaded &on_device(int device);      // (the caller has made `device` current)
    const std::string &arch() const { return arch_; }

private:
    Program() = default;
    std::string arch_;
    std::vector<char> code_;
    std::vector<double> data_;
    std::mutex mu_;
    std::map<int, Loaded> loaded_;
};

// rows a wavefront stages; the padded row stride in doubles (odd: the 32 lanes of one ds_read_b64
// group, each reading coordinate j of its own row, then fall into 32 different bank pairs)
constexpr int PROG_WAVE_ROWS = 64;
inline int prog_row_stride(int n) { return n | 1; }
inline size_t prog_stage_bytes(int n) { return (size_t) PROG_WAVE_ROWS * prog_row_stride(n) * sizeof(double); }
// the staged form is the default up to this n (set from the measurement)
constexpr int PROG_STAGE_MAX_N = 159;
constexpr size_t PROG_LDS_PER_CU = 160 * 1024;

// an engine's use of a program: the module on its device, the plan table, the one-row entry
class ProgEval {
public:
    ProgEval() = default;
    ProgEval(const ProgEval&) = delete;
    ProgEval& operator=(const ProgEval&) = delete;
    ~ProgEval();

    bool bound() const { return prog_ != nullptr; }
    // npop plan entries (+ the one-row entry behind them), for dimension n on `device` (current)
    void bind(const std::shared_ptr<Program> &prog, int device, int n, int npop);
    void unbind();
    void upload_plan(const std::vector<ProgPlan> &plan);
    // fills the table from device-side scalars (enqueued on st); X / f: the two halves of a double
    // buffer, pop_rows rows per population; which < 0: the half that is NOT current
    void fill_plan(hipStream_t st, const ProgScalView &sv, double *X0, double *X1, double *f0, double *f1,
            int pop_rows, int ld, int which, int rows, int honor_stop);
    // one launch over every population; stop != nullptr: a population whose flag (int at
    // stop + p * stop_stride bytes) is set is skipped
    void launch(hipStream_t st, int max_rows, const void *stop, int stop_stride, KernelTimer *timer);
    double evaluate_point(hipStream_t st, const double *x);

    void set_stage(int mode) { stage_ = mode; }      // -1 automatic, 0 direct, 1 staged
    int stage() const { return stage_; }
    bool staged() const;

private:
    std::shared_ptr<Program> prog_;
    Program::Loaded fn_;
    int n_ = 0, npop_ = 0;
    int stage_ = -1;
    ProgPlan *plan_ = nullptr;      // [npop + 1]
    double *xpoint_ = nullptr;      // [n] + [1]
};

} // namespace bbo
