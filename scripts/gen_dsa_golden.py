#!/usr/bin/env python3
"""Records states of the REAL DSSearch of the reference into tests/golden/dsa_runs.json
(needs the reference's sources and g++).

    python scripts/gen_dsa_golden.py [--ref /root/reference] [--out tests/golden/dsa_runs.json]

A small harness (the C++ text below, this project's own) is compiled in a temporary directory
against the reference's ds.cpp and blas.cpp with the flags of oracle/Makefile (-O2
-ffp-contract=off).  It seeds effolkronium::random_static::seed(k) and drives a subclass probe.

"steps": the state after init() and after each of the first 4 generations of six small shapes
(n in 1..6, np in 2..12 with np = 2, `adapt` on and off, nbatch = 2 so that the bandit's reset
shows; the seeds are chosen so that all four methods and all three map strategies occur).  Per
generation: the raw 32-bit words the generation takes from the global mt19937 -- exactly as many as
iterate() consumed, counted on a copy of the engine --, the method index (computed by the probe
BEFORE iterate(): with `adapt` on a copy of _generator and _p, else on a copy of the global engine),
and after iterate() the pool, _f, _so, _fso, _map, _dir, _w, _p, _it, _fev and converged().
tests/dsa_model.py turns the words into the reference's draws by the libstdc++ rules of SURVEY.md
Appendix C.
"bands": the sorted best f of 256 seeds (1000 + s) at a fixed budget (mfev = 4000, tol = stol = 0)
on the sphere and on Rosenbrock, n = 10, np = 40, default arguments, box [-5, 5].
"signature": the argument names and defaults of DSSearch's constructor (ds.h:60-61, bound at
py/multivariate_py.cpp:189-191).
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

# (name, n, np, adapt, nbatch, objective, box, seed)
STEPS = [
    ("n1_np2_adapt_b2", 1, 2, 1, 2, "sphere", 4., 51),
    ("n3_np7_adapt_b2", 3, 7, 1, 2, "rosenbrock", 3., 32),
    ("n6_np12_fixed", 6, 12, 0, 100, "ellipsoid", 5., 73),
    ("n2_np5_fixed", 2, 5, 0, 100, "rosenbrock", 2., 114),
    ("n4_np8_adapt_b100", 4, 8, 1, 100, "sphere", 5., 45),
    ("n5_np10_fixed_b2", 5, 10, 0, 2, "sphere", 5., 86),
]
GENERATIONS = 4
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
           "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}
BANDS = dict(n=10, np=40, mfev=4000, tol=0., stol=0., box=5., seed0=1000, count=256)
SIGNATURE = [{"name": "mfev", "required": True}, {"name": "tol", "required": True},
             {"name": "stol", "required": True}, {"name": "np", "required": True},
             {"name": "adapt", "required": False, "default": True},
             {"name": "nbatch", "required": False, "default": 100}]

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
#include <algorithm>
#include "objectives.h"
#include "random.hpp"
#include "multivariate/multivariate.h"
#define private protected          /* converged() is private in ds.h: the probe reads it */
#include "multivariate/pso/ds.h"
#undef private

using Random = effolkronium::random_static;

struct Probe: public DSSearch {
    using DSSearch::DSSearch;
    static void vec(const char *k, const std::vector<double> &v, bool last = false)
    {
        printf("\"%s\":[", k);
        for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
        printf("]%s", last ? "" : ",");
    }
    void dump(bool full)
    {
        std::vector<double> x, f, so, fso, dir;
        std::vector<int> map;
        for (auto &pt : _swarm) {
            x.insert(x.end(), pt._x.begin(), pt._x.end());
            so.insert(so.end(), pt._so.begin(), pt._so.end());
            dir.insert(dir.end(), pt._dir.begin(), pt._dir.end());
            map.insert(map.end(), pt._map.begin(), pt._map.end());
            f.push_back(pt._f);
            fso.push_back(pt._fso);
        }
        vec("X", x); vec("f", f); vec("w", _w); vec("p", _p);
        if (full) {
            vec("so", so); vec("fso", fso); vec("dir", dir);
            printf("\"map\":[");
            for (size_t i = 0; i < map.size(); i++) printf("%s%d", i ? "," : "", map[i]);
            printf("],");
        }
        printf("\"it\":%d,\"fev\":%d,\"converged\":%d", _it, _fev, converged() ? 1 : 0);
    }
    // the method index iterate() is about to draw, on copies of the engines it will use
    int next_method()
    {
        if (_adapt) {
            auto g = _generator;
            std::discrete_distribution<int> distribution(_p.begin(), _p.end());
            return distribution(g);
        }
        auto e = Random::get_engine();
        std::uniform_real_distribution<double> u(0.0, 0.3);
        u(e);
        u(e);
        std::uniform_int_distribution<int> k(0, 3);
        return k(e);
    }
    double best()
    {
        double b = _swarm[0]._f;
        for (auto &pt : _swarm) b = std::min(b, pt._f);
        return b;
    }
};

struct Ctx { int obj, n; std::vector<double> aux; };

int main(int argc, char **argv)
{
    // steps <obj> <n> <np> <adapt> <nbatch> <box> <seed> <generations>
    // bands <obj> <n> <np> <mfev> <tol> <stol> <box> <seed0> <count>
    Ctx c { atoi(argv[2]), atoi(argv[3]), {} };
    const int n = c.n;
    c.aux.resize(n);
    bbo_objective_aux(c.obj, n, c.aux.data());
    multivariate f = [&c](const double *x) { return bbo_objective_eval(c.obj, c.n, x, c.aux.data()); };
    if (!strcmp(argv[1], "steps")) {
        const double box = atof(argv[7]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed((unsigned) atoi(argv[8]));
        Probe p(1000000, 1e-12, 1e-12, atoi(argv[4]), atoi(argv[5]) != 0, atoi(argv[6]));
        p.init(prob, guess.data());
        printf("{\"init\":{");
        p.dump(false);
        printf("},\"states\":[");
        const int gens = atoi(argv[9]);
        for (int g = 1; g <= gens; g++) {
            const int im = p.next_method();
            auto before = Random::get_engine();
            p.iterate();
            const auto after = Random::get_engine();
            printf("%s{\"imethd\":%d,\"words\":[", g > 1 ? "," : "", im);
            for (int i = 0; !(before == after); i++) printf("%s%u", i ? "," : "", (unsigned) before());
            printf("],");
            p.dump(true);
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
            Probe p(atoi(argv[5]), atof(argv[6]), atof(argv[7]), atoi(argv[4]));
            p.optimize(prob, guess.data());
            out.push_back(p.best());
        }
        printf("{");
        Probe::vec("fbest", out, true);
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


def build(ref, tmp):
    src = os.path.join(ref, "src")
    with open(os.path.join(tmp, "harness.cpp"), "w") as fh:
        fh.write(HARNESS)
    exe = os.path.join(tmp, "harness")
    subprocess.check_call(
        ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I" + src,
         "-I" + os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(tmp, "harness.cpp"),
         os.path.join(src, "blas.cpp"), os.path.join(src, "multivariate/pso/ds.cpp"), "-lm"])
    return exe


def run_steps(exe, n, np_, adapt, nbatch, obj, box, seed):
    out = subprocess.check_output(
        [exe, "steps", str(OBJ_IDS[obj]), str(n), str(np_), str(adapt), str(nbatch), repr(box),
         str(seed), str(GENERATIONS)])
    return _norm(json.loads(out))


def generate(ref="/root/reference"):
    tmp = tempfile.mkdtemp(prefix="dsa_golden_")
    try:
        exe = build(ref, tmp)
        steps = []
        for name, n, np_, adapt, nbatch, obj, box, seed in STEPS:
            rec = run_steps(exe, n, np_, adapt, nbatch, obj, box, seed)
            rec.update({"name": name, "n": n, "np": np_, "adapt": adapt, "nbatch": nbatch,
                        "objective": obj, "box": box, "seed": seed, "tol": 1e-12, "stol": 1e-12})
            steps.append(rec)
        bands = dict(BANDS)
        b = BANDS
        for obj in ("sphere", "rosenbrock"):
            out = subprocess.check_output(
                [exe, "bands", str(OBJ_IDS[obj]), str(b["n"]), str(b["np"]), str(b["mfev"]),
                 repr(b["tol"]), repr(b["stol"]), repr(b["box"]), str(b["seed0"]), str(b["count"])])
            vals = sorted(float.fromhex(v) for v in json.loads(out)["fbest"])
            bands[obj] = [v.hex() for v in vals]
        return {"steps": steps, "bands": bands, "signature": SIGNATURE}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "dsa_runs.json"))
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.ref, "src")):
        sys.exit("the reference sources are not at %s" % a.ref)
    text = dumps(generate(a.ref))
    with open(a.out, "w") as fh:
        fh.write(text)
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
