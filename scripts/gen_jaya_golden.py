#!/usr/bin/env python3
"""Records states of the REAL JayaSearch of the reference into tests/golden/jaya_runs.json
(needs the reference's sources and g++).

    python scripts/gen_jaya_golden.py [--ref /root/reference] [--out tests/golden/jaya_runs.json]

A small harness (the C++ text below, this project's own) is compiled in a temporary directory
against the reference's jaya.cpp and blas.cpp with the flags of oracle/Makefile (-O2
-ffp-contract=off).  It seeds effolkronium::random_static::seed(k) and drives a subclass probe.

"steps": the first 3 generations of six small shapes (all four mutations, np % k != 0, k0 = 1,
k0 = nks, `adapt` on and off).  Per shape the state after init(); per generation the raw 32-bit
words the generation takes from the global mt19937 -- exactly as many as iterate() consumed,
counted on a copy of the engine -- and, after iterate(), the pool in slot order, _len, _k,
_xchaos, _pstrat, _perfindex, _best, _fgbest, _bestx, _fev and converged().  tests/jaya_model.py
turns the words into the reference's draws by the libstdc++ rules of SURVEY.md Appendix C.
"bands": the sorted final _fgbest of 256 seeds at a fixed budget (mfev = 4000, tol = 0) on the
sphere and on Rosenbrock, n = 10, np = 40, npmin = 5, default arguments, box [-5, 5].
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

MUTATIONS = ("original", "levy", "tent_map", "logistic")
# (name, n, np, npmin, adapt, k0, mutation, objective, box, seed)
STEPS = [
    ("original_n3_np7_k2", 3, 7, 2, 1, 2, "original", "sphere", 5., 21),
    ("levy_n4_np8_k3", 4, 8, 2, 1, 3, "levy", "rosenbrock", 3., 22),
    ("tent_n5_np10_k1_fixed", 5, 10, 3, 0, 1, "tent_map", "sphere", 5., 23),
    ("logistic_n2_np9_k4", 2, 9, 2, 1, 4, "logistic", "rosenbrock", 2., 24),
    ("logistic_n6_np12_k2_fixed", 6, 12, 4, 0, 2, "logistic", "ellipsoid", 5., 25),
    ("original_n1_np5_k5", 1, 5, 1, 1, 5, "original", "sphere", 4., 26),
]
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
           "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}
BANDS = dict(n=10, np=40, npmin=5, mfev=4000, tol=0., box=5., seed0=1000, count=256)

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>
#include <functional>
#include <string>
#include <iostream>
#include "objectives.h"
#include "random.hpp"
#include "multivariate/multivariate.h"
#define private protected          /* converged() is private in jaya.h: the probe reads it */
#include "multivariate/jaya/jaya.h"
#undef private

using Random = effolkronium::random_static;

struct Probe: public JayaSearch {
    using JayaSearch::JayaSearch;
    static void vec(const char *k, const std::vector<double> &v, bool last = false)
    {
        printf("\"%s\":[", k);
        for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
        printf("]%s", last ? "" : ",");
    }
    void dump()
    {
        std::vector<double> x, f, len;
        for (auto &pt : _pool) {
            x.insert(x.end(), pt._x.begin(), pt._x.end());
            f.push_back(pt._f);
        }
        for (int q = 0; q < _k_used; q++) len.push_back(_len[q]);
        vec("X", x); vec("f", f); vec("len", len); vec("pstrat", _pstrat); vec("perfindex", _perfindex);
        vec("bestx", _bestx); vec("xchaos", { _xchaos }); vec("best", { _best }); vec("fgbest", { _fgbest });
        printf("\"k\":%d,\"fev\":%d,\"converged\":%d", _k, _fev, converged() ? 1 : 0);
    }
    void step()
    {
        _k_used = _k;
        iterate();
    }
    double fgbest() const { return _fgbest; }
    int _k_used = 0;
};

struct Ctx { int obj, n; std::vector<double> aux; };

int main(int argc, char **argv)
{
    // steps <obj> <n> <np> <npmin> <adapt> <k0> <mutation> <box> <seed>
    // bands <obj> <n> <np> <npmin> <mfev> <tol> <box> <seed0> <count>
    Ctx c { atoi(argv[2]), atoi(argv[3]), {} };
    const int n = c.n;
    c.aux.resize(n);
    bbo_objective_aux(c.obj, n, c.aux.data());
    multivariate f = [&c](const double *x) { return bbo_objective_eval(c.obj, c.n, x, c.aux.data()); };
    if (!strcmp(argv[1], "steps")) {
        const double box = atof(argv[9]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed((unsigned) atoi(argv[10]));
        Probe p(1000000, 1e-12, atoi(argv[4]), atoi(argv[5]), atoi(argv[6]) != 0, atoi(argv[7]),
                (JayaSearch::jaya_mutation_method) atoi(argv[8]));
        p.init(prob, guess.data());
        printf("{\"init\":{");
        p.dump();
        printf("},\"states\":[");
        for (int g = 1; g <= 3; g++) {
            auto before = Random::get_engine();
            p.step();
            const auto after = Random::get_engine();
            printf("%s{\"words\":[", g > 1 ? "," : "");
            for (int i = 0; !(before == after); i++) printf("%s%u", i ? "," : "", (unsigned) before());
            printf("],");
            p.dump();
            printf("}");
        }
        printf("]}\n");
    } else {
        const double box = atof(argv[8]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        const int seed0 = atoi(argv[9]), count = atoi(argv[10]);
        std::vector<double> out;
        for (int s = 0; s < count; s++) {
            Random::seed((unsigned) (seed0 + s));
            Probe p(atoi(argv[6]), atof(argv[7]), atoi(argv[4]), atoi(argv[5]));
            p.optimize(prob, guess.data());
            out.push_back(p.fgbest());
        }
        printf("{");
        Probe::vec("fgbest", out, true);
        printf("}\n");
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


def generate(ref="/root/reference"):
    src = os.path.join(ref, "src")
    tmp = tempfile.mkdtemp(prefix="jaya_golden_")
    try:
        with open(os.path.join(tmp, "harness.cpp"), "w") as fh:
            fh.write(HARNESS)
        exe = os.path.join(tmp, "harness")
        subprocess.check_call(
            ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I" + src,
             "-I" + os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(tmp, "harness.cpp"),
             os.path.join(src, "blas.cpp"), os.path.join(src, "multivariate/jaya/jaya.cpp"), "-lm"])
        steps = []
        for name, n, np_, npmin, adapt, k0, mut, obj, box, seed in STEPS:
            out = subprocess.check_output(
                [exe, "steps", str(OBJ_IDS[obj]), str(n), str(np_), str(npmin), str(adapt), str(k0),
                 str(MUTATIONS.index(mut)), repr(box), str(seed)])
            rec = _norm(json.loads(out))
            rec.update({"name": name, "n": n, "np": np_, "npmin": npmin, "adapt": adapt, "k0": k0,
                        "mutation": mut, "objective": obj, "box": box, "seed": seed,
                        "scale": 0.01, "beta": 1.5, "temper": 10.0, "tol": 1e-12})
            steps.append(rec)
        bands = dict(BANDS)
        b = BANDS
        for obj in ("sphere", "rosenbrock"):
            out = subprocess.check_output(
                [exe, "bands", str(OBJ_IDS[obj]), str(b["n"]), str(b["np"]), str(b["npmin"]),
                 str(b["mfev"]), repr(b["tol"]), repr(b["box"]), str(b["seed0"]), str(b["count"])])
            vals = sorted(float.fromhex(v) for v in json.loads(out)["fgbest"])
            bands[obj] = [v.hex() for v in vals]
        return {"steps": steps, "bands": bands}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "jaya_runs.json"))
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.ref, "src")):
        sys.exit("the reference sources are not at %s" % a.ref)
    text = dumps(generate(a.ref))
    with open(a.out, "w") as fh:
        fh.write(text)
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
