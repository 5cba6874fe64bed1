#!/usr/bin/env python3
"""Records states of the REAL Hees of the reference into tests/golden/hees_runs.json (needs the
reference's sources and g++).

    python scripts/gen_hees_golden.py [--ref /root/reference] [--out tests/golden/hees_runs.json]
    python scripts/gen_hees_golden.py --time        # the reference's ms per generation, one core

A small harness (the C++ text below, this project's own) is compiled in a temporary directory
against the reference's hees.cpp and blas.cpp with the flags of oracle/Makefile (-O2
-ffp-contract=off).  It seeds effolkronium::random_static::seed(k) and drives a subclass probe (all
members of Hees are protected; its normal distribution `_Z` is public).

"steps": the state after init() and after each of the first 4 generations of six small shapes,
(n, np) = (1, 0), (2, 0), (3, 7), (5, 5), (6, 0), (8, 3): B = 2 at n = 1, a partial last batch,
mu = n, mu < n.  Per generation: the raw 32-bit words the generation takes from the global mt19937
-- exactly as many as iterate() consumed, counted on a copy of the engine -- and after iterate() A,
the mean, sigma, p_s, g_s, all B n rows of b and their norms, the 2 mu candidates, their values and
ranks, h, q, f(m), the incumbent, fev and converged().  The polar method's spare normal lives in
`_Z` across generations; tests/hees_model.py keeps it too (jaya_model.Words.normal).  The start
points are off the origin so that no mirrored pair ties (std::sort leaves ties undefined).
"runs": two optimize() calls with mres = 3 and print = True at n = 4: every word consumed, the
table the reference printed, and the solution.
"bands": the sorted final fbest of 256 seeds (1000 + s) at a fixed budget on the sphere and on
Rosenbrock, n = 10, default arguments (mres = 1, np = 0, sigma0 = 2), tol = 0, every coordinate
of the guess 3.
"signature": the argument names and defaults of Hees's constructor (hees.h:70-71, bound at
py/multivariate_py.cpp:206-211).
Floats are float.hex strings.  The fixture holds numbers and names only.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, n, np, objective, box, seed, sigma0)
STEPS = [
    ("n1_np0", 1, 0, "sphere", 4., 11, 2.),
    ("n2_np0", 2, 0, "rosenbrock", 3., 22, 2.),
    ("n3_np7", 3, 7, "ellipsoid", 5., 33, 1.),
    ("n5_np5", 5, 5, "rosenbrock", 5., 44, 2.),
    ("n6_np0", 6, 0, "sphere", 5., 55, 0.5),
    ("n8_np3", 8, 3, "ellipsoid", 5., 66, 2.),
]
GENERATIONS = 4
# (name, n, np, objective, box, seed, mfev, tol, mres, sigma0)
RUNS = [
    ("n4_np0_mres3_rosenbrock", 4, 0, "rosenbrock", 5., 77, 700, 1., 3, 2.),
    ("n4_np6_mres3_sphere", 4, 6, "sphere", 5., 88, 800, 1e-1, 3, 1.),
]
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
           "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}
BANDS = dict(n=10, mfev=1500, tol=0., box=5., guess=3., seed0=1000, count=256)
SIGNATURE = [{"name": "mfev", "required": True}, {"name": "tol", "required": True},
             {"name": "mres", "required": False, "default": 1},
             {"name": "print", "required": False, "default": False},
             {"name": "np", "required": False, "default": 0},
             {"name": "sigma0", "required": False, "default": 2.}]


def guess_of(n, base=0.5):
    """the start point of "steps" and "runs": off the origin and off every symmetry"""
    return [base + 0.25 * j for j in range(n)]


HARNESS = r"""
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>
#include <functional>
#include <string>
#include <iostream>
#include <algorithm>
#include <numeric>
#include "objectives.h"
#include "random.hpp"
#include "tabular.hpp"
#include "multivariate/multivariate.h"
#define private protected          /* converged() is private in hees.h: the probe reads it */
#include "multivariate/hees/hees.h"
#undef private

using Random = effolkronium::random_static;

struct Probe: public Hees {
    using Hees::Hees;
    static void vec(FILE *o, const char *k, const std::vector<double> &v, bool last = false)
    {
        fprintf(o, "\"%s\":[", k);
        for (size_t i = 0; i < v.size(); i++) fprintf(o, "%s\"%a\"", i ? "," : "", v[i]);
        fprintf(o, "]%s", last ? "" : ",");
    }
    static std::vector<double> flat(const std::vector<std::vector<double>> &m)
    {
        std::vector<double> v;
        for (auto &r : m) v.insert(v.end(), r.begin(), r.end());
        return v;
    }
    void dump()
    {
        std::vector<double> fv;
        std::vector<int> rk;
        for (auto &pt : _fitness) {
            fv.push_back(pt._value);
            rk.push_back(pt._rank);
        }
        vec(stdout, "A", flat(_a)); vec(stdout, "xmean", _xmean); vec(stdout, "ps", _ps);
        vec(stdout, "b", flat(_b)); vec(stdout, "norms", _norms); vec(stdout, "x", flat(_x));
        vec(stdout, "fit_val", fv); vec(stdout, "hess", _hess); vec(stdout, "q", _q);
        vec(stdout, "xbest", _xbest); vec(stdout, "weights", _weights);
        vec(stdout, "scalars", { _sigma, _gs, _fm, _fbest, _cs, _ds, _chi, _mueff, _mueffm });
        printf("\"rank\":[");
        for (size_t i = 0; i < rk.size(); i++) printf("%s%d", i ? "," : "", rk[i]);
        printf("],\"mu\":%d,\"B\":%d,\"fev\":%d,\"converged\":%d", _mu, _B, _fev, converged() ? 1 : 0);
    }
    double fbest() const { return _fbest; }
};

struct Ctx { int obj, n; std::vector<double> aux; };

int main(int argc, char **argv)
{
    // steps <obj> <n> <np> <box> <seed> <generations> <sigma0> <guess0>
    // runs  <obj> <n> <np> <box> <seed> <mfev> <tol> <mres> <sigma0> <guess0>   (JSON on stderr)
    // bands <obj> <n> <mfev> <tol> <box> <guess> <seed0> <count>
    // time  <obj> <n> <np> <generations>
    Ctx c { atoi(argv[2]), atoi(argv[3]), {} };
    const int n = c.n;
    c.aux.resize(n);
    bbo_objective_aux(c.obj, n, c.aux.data());
    multivariate f = [&c](const double *x) { return bbo_objective_eval(c.obj, c.n, x, c.aux.data()); };
    if (!strcmp(argv[1], "steps")) {
        const double box = atof(argv[5]), g0 = atof(argv[9]);
        std::vector<double> lo(n, -box), up(n, box), guess(n);
        for (int j = 0; j < n; j++) guess[j] = g0 + 0.25 * j;
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed((unsigned) atoi(argv[6]));
        Probe p(1000000, 1e-12, 1, false, atoi(argv[4]), atof(argv[8]));
        p.init(prob, guess.data());
        printf("{\"init\":{");
        p.dump();
        printf("},\"states\":[");
        const int gens = atoi(argv[7]);
        for (int g = 1; g <= gens; g++) {
            auto before = Random::get_engine();
            p.iterate();
            const auto after = Random::get_engine();
            printf("%s{\"words\":[", g > 1 ? "," : "");
            for (int i = 0; !(before == after); i++) printf("%s%u", i ? "," : "", (unsigned) before());
            printf("],");
            p.dump();
            printf("}");
        }
        printf("]}\n");
    } else if (!strcmp(argv[1], "runs")) {
        const double box = atof(argv[5]), g0 = atof(argv[11]);
        std::vector<double> lo(n, -box), up(n, box), guess(n);
        for (int j = 0; j < n; j++) guess[j] = g0 + 0.25 * j;
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed((unsigned) atoi(argv[6]));
        Probe p(atoi(argv[7]), atof(argv[8]), atoi(argv[9]), true, atoi(argv[4]), atof(argv[10]));
        auto before = Random::get_engine();
        const auto sol = p.optimize(prob, guess.data());
        const auto after = Random::get_engine();
        std::cout.flush();
        fprintf(stderr, "{\"words\":[");
        for (int i = 0; !(before == after); i++) fprintf(stderr, "%s%u", i ? "," : "", (unsigned) before());
        fprintf(stderr, "],");
        Probe::vec(stderr, "x", sol._sol);
        fprintf(stderr, "\"n_evals\":%d,\"converged\":%d}\n", sol._fev, sol._converged ? 1 : 0);
    } else if (!strcmp(argv[1], "bands")) {
        const double box = atof(argv[6]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, atof(argv[7]));
        multivariate_problem prob { f, n, lo.data(), up.data() };
        const int seed0 = atoi(argv[8]), count = atoi(argv[9]);
        std::vector<double> out;
        for (int s = 0; s < count; s++) {
            Random::seed((unsigned) (seed0 + s));
            Probe p(atoi(argv[4]), atof(argv[5]));
            p.optimize(prob, guess.data());
            out.push_back(p.fbest());
        }
        printf("{");
        Probe::vec(stdout, "fbest", out, true);
        printf("}\n");
    } else {
        std::vector<double> lo(n, -5.), up(n, 5.), guess(n, 3.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed(1u);
        Probe p(1 << 30, 0., 1, false, atoi(argv[4]), 2.);
        p.init(prob, guess.data());
        const int gens = atoi(argv[5]);
        p.iterate();
        const auto t0 = std::chrono::steady_clock::now();
        for (int g = 0; g < gens; g++) p.iterate();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("{\"ms_per_generation\":%.6f}\n", ms / gens);
    }
    return 0;
}
"""


def _norm(obj):
    """hex strings as Python writes them (the C library's %a may choose another normalisation)"""
    if isinstance(obj, dict):
        return {k: _norm(v) for k, v in obj.items()}
    if isinstance(obj, list):
        return [_norm(v) for v in obj]
    if isinstance(obj, str) and ("0x" in obj or obj in ("inf", "-inf", "nan", "-nan")):
        return float.fromhex(obj).hex() if "0x" in obj else float(obj.replace("-nan", "nan")).hex()
    return obj


def build(ref, tmp):
    src = os.path.join(ref, "src")
    with open(os.path.join(tmp, "harness.cpp"), "w") as fh:
        fh.write(HARNESS)
    exe = os.path.join(tmp, "harness")
    subprocess.check_call(
        ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I" + src,
         "-I" + os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(tmp, "harness.cpp"),
         os.path.join(src, "blas.cpp"), os.path.join(src, "multivariate/hees/hees.cpp"), "-lm"])
    return exe


def generate(ref="/root/reference"):
    tmp = tempfile.mkdtemp(prefix="hees_golden_")
    try:
        exe = build(ref, tmp)
        steps = []
        for name, n, np_, obj, box, seed, sigma0 in STEPS:
            out = subprocess.check_output(
                [exe, "steps", str(OBJ_IDS[obj]), str(n), str(np_), repr(box), str(seed),
                 str(GENERATIONS), repr(sigma0), "0.5"])
            rec = _norm(json.loads(out))
            rec.update({"name": name, "n": n, "np": np_, "objective": obj, "box": box, "seed": seed,
                        "sigma0": sigma0, "tol": 1e-12, "guess": [v.hex() for v in guess_of(n)]})
            steps.append(rec)
        runs = []
        for name, n, np_, obj, box, seed, mfev, tol, mres, sigma0 in RUNS:
            pr = subprocess.run(
                [exe, "runs", str(OBJ_IDS[obj]), str(n), str(np_), repr(box), str(seed), str(mfev),
                 repr(tol), str(mres), repr(sigma0), "0.5"], check=True, capture_output=True, text=True)
            rec = _norm(json.loads(pr.stderr))
            rec.update({"name": name, "n": n, "np": np_, "objective": obj, "box": box, "seed": seed,
                        "mfev": mfev, "tol": tol, "mres": mres, "sigma0": sigma0,
                        "guess": [v.hex() for v in guess_of(n)], "table": pr.stdout.splitlines()})
            runs.append(rec)
        bands = dict(BANDS)
        b = BANDS
        for obj in ("sphere", "rosenbrock"):
            out = subprocess.check_output(
                [exe, "bands", str(OBJ_IDS[obj]), str(b["n"]), str(b["mfev"]), repr(b["tol"]),
                 repr(b["box"]), repr(b["guess"]), str(b["seed0"]), str(b["count"])])
            vals = sorted(float.fromhex(v) for v in json.loads(out)["fbest"])
            bands[obj] = [v.hex() for v in vals]
        return {"steps": steps, "runs": runs, "bands": bands, "signature": SIGNATURE}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def time_reference(ref="/root/reference"):
    """ms per generation of the reference on one core: the two population shapes of scripts/bench_hees.py"""
    tmp = tempfile.mkdtemp(prefix="hees_time_")
    try:
        exe = build(ref, tmp)
        for n, np_, gens in ((128, 0, 20), (128, 2048, 1)):
            out = json.loads(subprocess.check_output(
                [exe, "time", str(OBJ_IDS["rosenbrock"]), str(n), str(np_), str(gens)]))
            print("n = %d, np = %d: %.3f ms per generation" % (n, np_, out["ms_per_generation"]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "hees_runs.json"))
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.ref, "src")):
        sys.exit("the reference sources are not at %s" % a.ref)
    if a.time:
        time_reference(a.ref)
        return
    text = dumps(generate(a.ref))
    with open(a.out, "w") as fh:
        fh.write(text)
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
