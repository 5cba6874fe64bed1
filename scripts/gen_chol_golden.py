#!/usr/bin/env python3
"""Records states of the REAL CholeskyCmaes of the reference into tests/golden/chol_runs.json
(needs the reference's sources and g++).

    python scripts/gen_chol_golden.py [--ref /root/reference] [--out tests/golden/chol_runs.json]

A small harness (the C++ text below, this project's own) is compiled in a temporary directory
against the reference's base_cmaes.cpp, cholesky_cmaes.cpp and blas.cpp with the flags of
oracle/Makefile (-O2 -ffp-contract=off).  It seeds effolkronium::random_static::seed(k), drives a
subclass probe generation by generation and prints, per generation: the normals the sampler is
about to draw, arx, fit_val, fit_idx, xmean, sigma, pc, ps, A, it, fev, converged().  Floats are
float.hex strings (tests/_golden.py).  The fixture holds numbers and names only.

"steps": the first 3 generations of six shapes (n in {2, 5, 10, 16}; lambda < 2 n and >= 4 n;
`bound` on and off, one bounded run starting next to a corner).  n = 16 with lambda >= 4 n is
left out: it alone would take the fixture past its 300 KB.
"runs": outcome (generations, fev, converged, final best f) of complete runs on the sphere,
n = 5, lambda = 12, tol = stol = 1e-8, for 16 seeds.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, n, lambda, objective, bound, box, seed, start)   start: "mid" or "corner"
STEPS = [
    ("n2_l8_sphere", 2, 8, "sphere", 0, 5., 11, "mid"),
    ("n5_l8_rosenbrock", 5, 8, "rosenbrock", 0, 5., 12, "mid"),
    ("n5_l20_ellipsoid_box_corner", 5, 20, "ellipsoid", 1, 3., 13, "corner"),
    ("n10_l12_ellipsoid", 10, 12, "ellipsoid", 0, 5., 14, "mid"),
    ("n10_l40_rosenbrock_box", 10, 40, "rosenbrock", 1, 4., 15, "mid"),
    ("n16_l24_cigar", 16, 24, "cigar", 0, 5., 16, "mid"),
]
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
           "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}
RUN_SEEDS = list(range(101, 117))

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "objectives.h"
#include "random.hpp"
#include "multivariate/cma/cholesky_cmaes.h"

using Random = effolkronium::random_static;

struct Probe: public CholeskyCmaes {
    using CholeskyCmaes::CholeskyCmaes;
    void vec(const char *k, const std::vector<double> &v, bool last = false)
    {
        printf("\"%s\":[", k);
        for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
        printf("]%s", last ? "" : ",");
    }
    void peek()
    {
        auto eng = Random::get_engine();
        auto dist = _Z;
        std::vector<double> z((size_t) _lambda * _n);
        for (auto &v : z) v = dist(eng);
        vec("normals", z);
    }
    void dump(int gen)
    {
        std::vector<double> arx, fv, fi, a;
        for (auto &r : _arx) arx.insert(arx.end(), r.begin(), r.end());
        for (auto &f : _fitness) { fv.push_back(f._value); fi.push_back(f._index); }
        for (auto &r : _a) a.insert(a.end(), r.begin(), r.end());
        printf("\"gen\":%d,", gen);
        vec("arx", arx); vec("fit_val", fv); vec("fit_idx", fi); vec("xmean", _xmean);
        vec("sigma", { _sigma }); vec("pc", _pc); vec("ps", _ps); vec("A", a);
        printf("\"it\":%d,\"fev\":%d,\"converged\":%d", _it, _fev, converged() ? 1 : 0);
    }
    int its() const { return _it; }
    double fbest() const { return _ybw[0]; }
};

struct Ctx { int obj, n; std::vector<double> aux; };

int main(int argc, char **argv)
{
    // steps <obj> <n> <lambda> <bound> <box> <seed> <corner> <mfev> <tol> <stol>
    // run   <seed>
    if (!strcmp(argv[1], "steps")) {
        Ctx c { atoi(argv[2]), atoi(argv[3]), {} };
        const int n = c.n, lambda = atoi(argv[4]), bound = atoi(argv[5]);
        const double box = atof(argv[6]);
        const int corner = atoi(argv[8]);
        c.aux.resize(n);
        bbo_objective_aux(c.obj, n, c.aux.data());
        Random::seed((unsigned) atoi(argv[7]));
        std::vector<double> lo(n, -box), up(n, box), guess(n);
        for (int i = 0; i < n; i++)
            guess[i] = corner ? box - 0.05 * (1 + i % 3) : Random::get(-0.6 * box, 0.6 * box);
        multivariate f = [&c](const double *x) { return bbo_objective_eval(c.obj, c.n, x, c.aux.data()); };
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Probe p(atoi(argv[9]), atof(argv[10]), atof(argv[11]), lambda, 2., bound != 0);
        p.init(prob, guess.data());
        printf("{");
        p.vec("guess", guess);
        printf("\"states\":[");
        for (int g = 1; g <= 3; g++) {
            printf("%s{", g > 1 ? "," : "");
            p.peek();
            p.iterate();
            p.dump(g);
            printf("}");
        }
        printf("]}\n");
    } else {
        Ctx c { BBO_OBJ_SPHERE, 5, std::vector<double>(5, 0.) };
        const int n = 5;
        Random::seed((unsigned) atoi(argv[2]));
        std::vector<double> lo(n, -10.), up(n, 10.), guess(n);
        for (int i = 0; i < n; i++) guess[i] = Random::get(-3., 3.);
        multivariate f = [&c](const double *x) { return bbo_objective_eval(c.obj, c.n, x, c.aux.data()); };
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Probe p(100000, 1e-8, 1e-8, 12, 2., false);
        const auto sol = p.optimize(prob, guess.data());
        printf("{\"seed\":%d,\"generations\":%d,\"fev\":%d,\"converged\":%d,\"f\":\"%a\"}\n",
                atoi(argv[2]), p.its(), sol._fev, sol._converged ? 1 : 0, p.fbest());
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
    if isinstance(obj, str) and ("0x" in obj or obj in ("inf", "-inf", "nan")):
        return float.fromhex(obj).hex()
    return obj


def generate(ref="/root/reference"):
    src = os.path.join(ref, "src")
    tmp = tempfile.mkdtemp(prefix="chol_golden_")
    try:
        with open(os.path.join(tmp, "harness.cpp"), "w") as fh:
            fh.write(HARNESS)
        exe = os.path.join(tmp, "harness")
        subprocess.check_call(
            ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I" + src,
             "-I" + os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(tmp, "harness.cpp"),
             os.path.join(src, "blas.cpp"), os.path.join(src, "multivariate/cma/base_cmaes.cpp"),
             os.path.join(src, "multivariate/cma/cholesky_cmaes.cpp"), "-lm"])
        steps = []
        for name, n, lam, obj, bound, box, seed, start in STEPS:
            mfev, tol, stol = 1000 * lam, 1e-12, 1e-12
            out = subprocess.check_output(
                [exe, "steps", str(OBJ_IDS[obj]), str(n), str(lam), str(bound), repr(box), str(seed),
                 "1" if start == "corner" else "0", str(mfev), repr(tol), repr(stol)])
            rec = _norm(json.loads(out))
            rec.update({"name": name, "n": n, "lambda": lam, "objective": obj, "bound": bound,
                        "box": box, "seed": seed, "mfev": mfev, "tol": tol, "stol": stol,
                        "sigma0": 2.0})
            steps.append(rec)
        runs = [_norm(json.loads(subprocess.check_output([exe, "run", str(s)]))) for s in RUN_SEEDS]
        return {"steps": steps,
                "runs": {"objective": "sphere", "n": 5, "lambda": 12, "tol": 1e-8, "stol": 1e-8,
                         "sigma0": 2.0, "mfev": 100000, "results": runs}}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "chol_runs.json"))
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.ref, "src")):
        sys.exit("the reference sources are not at %s" % a.ref)
    text = dumps(generate(a.ref))
    with open(a.out, "w") as fh:
        fh.write(text)
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
