#!/usr/bin/env python3
"""Records states of the REAL SpiralSearch of the reference into tests/golden/spiral_runs.json
(needs the reference's sources and g++).

    python scripts/gen_spiral_golden.py [--ref /root/reference] [--out tests/golden/spiral_runs.json]
    python scripts/gen_spiral_golden.py --time      # the reference's ms per generation, one core

A small harness (the C++ text below, this project's own) is compiled in a temporary directory
against the reference's spiral.cpp with the flags of oracle/Makefile (-O2 -ffp-contract=off).  It
seeds effolkronium::random_static::seed(k) and drives a subclass probe (the members of SpiralSearch
are protected).

"steps": the state after init() and after each of the first 4 generations of six small shapes,
(n, np) = (1, 3), (2, 5), (3, 7), (5, 20), (9, 20), (17, 4): the points, their values, rs, thetas,
ibest, xbest and fev.  Every shape is recorded twice: with taur = tautheta = 0 (name *_fixed: the
trajectory depends on nothing but the initial points) and with taur = tautheta = 0.5 (name *_adapt),
where each generation also carries the raw 32-bit words it took from the global mt19937 -- exactly
as many as iterate() consumed, counted on a copy of the engine.  The generator asserts that in
every recorded state the best value and the runner-up differ by more than 1e-6 relative, so that
no comparison against the fixture can turn on an arg-min flip; a seed that fails is replaced.
"bands": the sorted final f(xbest) of 256 seeds (1000 + s) at a fixed budget on the sphere and on
Rosenbrock, n = 10, default arguments.
"signature": the argument names and defaults of SpiralSearch's constructor as bound at
py/multivariate_py.cpp:344-351.
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

# (name, n, np, objective, box, seed)
SHAPES = [
    ("n1_np3", 1, 3, "sphere", 4., 11),
    ("n2_np5", 2, 5, "rosenbrock", 3., 22),
    ("n3_np7", 3, 7, "ellipsoid", 5., 33),
    ("n5_np20", 5, 20, "rosenbrock", 5., 44),
    ("n9_np20", 9, 20, "sphere", 5., 55),
    ("n17_np4", 17, 4, "ellipsoid", 5., 66),
]
# (suffix, taur, tautheta)
MODES = [("fixed", 0., 0.), ("adapt", 0.5, 0.5)]
GENERATIONS = 4
MIN_GAP = 1e-6
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
           "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}
BANDS = dict(n=10, mfev=4000, tol=0., box=5., seed0=1000, count=256)
SIGNATURE = [{"name": "mfev", "required": True}, {"name": "tol", "required": True},
             {"name": "np", "required": False, "default": 20},
             {"name": "r", "required": False, "default": 0.95},
             {"name": "theta", "required": False, "default": 1.57079632679},
             {"name": "taur", "required": False, "default": 0.0},
             {"name": "tautheta", "required": False, "default": 0.1},
             {"name": "rlow", "required": False, "default": 0.9},
             {"name": "rhigh", "required": False, "default": 1.0},
             {"name": "thetalow", "required": False, "default": 0.0},
             {"name": "thetahigh", "required": False, "default": 6.28318530718}]

HARNESS = r"""
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <random>
#include <string>
#include <vector>
#include "objectives.h"
#include "random.hpp"
#include "multivariate/multivariate.h"
#include "multivariate/spiral/spiral.h"

using Random = effolkronium::random_static;

struct Probe: public SpiralSearch {
    using SpiralSearch::SpiralSearch;
    static void vec(const char *k, const std::vector<double> &v, bool last = false)
    {
        printf("\"%s\":[", k);
        for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
        printf("]%s", last ? "" : ",");
    }
    void dump()
    {
        std::vector<double> pts;
        for (auto &r : _points) pts.insert(pts.end(), r.begin(), r.end());
        vec("x", pts); vec("f", _fs); vec("rs", _rs); vec("thetas", _thetas); vec("xbest", _xbest);
        printf("\"ibest\":%d,\"fev\":%d", _ibest, _fev);
    }
    double fbest() const { return _fs[_ibest]; }
};

struct Ctx { int obj, n; std::vector<double> aux; };

int main(int argc, char **argv)
{
    // steps <obj> <n> <np> <box> <seed> <generations> <taur> <tautheta>
    // bands <obj> <n> <mfev> <tol> <box> <seed0> <count>
    // time  <obj> <n> <np> <generations>
    Ctx c { atoi(argv[2]), atoi(argv[3]), {} };
    const int n = c.n;
    c.aux.resize(n);
    bbo_objective_aux(c.obj, n, c.aux.data());
    multivariate f = [&c](const double *x) { return bbo_objective_eval(c.obj, c.n, x, c.aux.data()); };
    if (!strcmp(argv[1], "steps")) {
        const double box = atof(argv[5]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed((unsigned) atoi(argv[6]));
        Probe p(1000000, 0., atoi(argv[4]), 0.95, 1.57079632679, atof(argv[8]), atof(argv[9]), 0.9, 1.0, 0.0,
                6.28318530718);
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
    } else if (!strcmp(argv[1], "bands")) {
        const double box = atof(argv[6]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        const int seed0 = atoi(argv[7]), count = atoi(argv[8]);
        std::vector<double> out;
        for (int s = 0; s < count; s++) {
            Random::seed((unsigned) (seed0 + s));
            Probe p(atoi(argv[4]), atof(argv[5]), 20, 0.95, 1.57079632679, 0.0, 0.1, 0.9, 1.0, 0.0, 6.28318530718);
            p.optimize(prob, guess.data());
            out.push_back(p.fbest());
        }
        printf("{");
        Probe::vec("fbest", out, true);
        printf("}\n");
    } else {
        std::vector<double> lo(n, -5.), up(n, 5.), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed(1u);
        Probe p(1 << 30, 0., atoi(argv[4]), 0.95, 1.57079632679, 0.0, 0.1, 0.9, 1.0, 0.0, 6.28318530718);
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
        ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-include", "cmath", "-I" + src,
         "-I" + os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(tmp, "harness.cpp"),
         os.path.join(src, "multivariate/spiral/spiral.cpp"), "-lm"])
    return exe


def gap_ok(state):
    """the best value and the runner-up differ by more than MIN_GAP relative"""
    f = sorted(float.fromhex(v) for v in state["f"])
    return len(f) < 2 or abs(f[1] - f[0]) > MIN_GAP * max(abs(f[0]), abs(f[1]))


def record(exe, name, n, np_, obj, box, seed, taur, tautheta):
    """one shape; the seed moves on until no recorded state has a near-tie for the best"""
    for attempt in range(64):
        out = subprocess.check_output(
            [exe, "steps", str(OBJ_IDS[obj]), str(n), str(np_), repr(box), str(seed + 1000 * attempt),
             str(GENERATIONS), repr(taur), repr(tautheta)])
        rec = _norm(json.loads(out))
        if all(gap_ok(s) for s in [rec["init"]] + rec["states"]):
            break
    else:
        sys.exit("%s: no seed without a near-tie" % name)
    assert all(gap_ok(s) for s in [rec["init"]] + rec["states"]), name
    rec.update({"name": name, "n": n, "np": np_, "objective": obj, "box": box, "seed": seed + 1000 * attempt,
                "taur": taur, "tautheta": tautheta})
    return rec


def generate(ref="/root/reference"):
    tmp = tempfile.mkdtemp(prefix="spiral_golden_")
    try:
        exe = build(ref, tmp)
        steps = []
        for name, n, np_, obj, box, seed in SHAPES:
            for suffix, taur, tautheta in MODES:
                steps.append(record(exe, name + "_" + suffix, n, np_, obj, box, seed, taur, tautheta))
        bands = dict(BANDS)
        b = BANDS
        for obj in ("sphere", "rosenbrock"):
            out = subprocess.check_output(
                [exe, "bands", str(OBJ_IDS[obj]), str(b["n"]), str(b["mfev"]), repr(b["tol"]),
                 repr(b["box"]), str(b["seed0"]), str(b["count"])])
            vals = sorted(float.fromhex(v) for v in json.loads(out)["fbest"])
            bands[obj] = [v.hex() for v in vals]
        return {"steps": steps, "bands": bands, "signature": SIGNATURE}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def time_reference(ref="/root/reference"):
    """ms per generation of the reference on one core: the two population shapes of scripts/bench_spiral.py"""
    tmp = tempfile.mkdtemp(prefix="spiral_time_")
    try:
        exe = build(ref, tmp)
        for n, np_, gens in ((128, 20, 50), (128, 4096, 2)):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "spiral_runs.json"))
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
