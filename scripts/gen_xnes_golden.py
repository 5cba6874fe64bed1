#!/usr/bin/env python3
"""Records states of the REAL xNES of the reference into tests/golden/xnes_runs.json (needs the
reference's sources and g++).

    python scripts/gen_xnes_golden.py [--ref /root/reference] [--out tests/golden/xnes_runs.json]
    python scripts/gen_xnes_golden.py --time      (ms per generation of the reference at n = 128 and 512
                                                   on one host core, for scripts/bench_xnes.py's lines)

A small harness (the C++ text below, this project's own) is compiled in a temporary directory
against the reference's xnes.cpp and blas.cpp with the flags of oracle/Makefile (-O2
-ffp-contract=off).  It seeds effolkronium::random_static::seed(k) and drives a probe subclass
generation by generation.  Before every generation the probe copies the engine and the class's
normal distribution and replays the np * n draws the sampler is about to make (`z`, sampling
order).  The fixture holds numbers and names only; an array of floats is ONE string, base64 of its
little-endian IEEE doubles (tests/test_xnes_model.py, `unpack`), the scalar outcomes of "runs" are
float.hex strings.

"steps": four runs (STEPS below: n = 2, 5, 12 on the dense route of the device, n = 33 on the
low-rank one); every generation keeps its draws, the listed generations the whole state: arx and
fit_val as the class holds them (ranked), fit_idx (the sampling index of every ranked point, found
by matching its z to the draws), xmean, sigma, gsigma, B, it, fev.
"runs": outcomes (fev, converged, f of the returned point) of complete runs: 16 seeds of Rosenbrock
n = 10, tol = 1e-8, and one run that ends on the budget.

The seed of a "steps" run is advanced until no two fitness values of a recorded generation are
closer than 1e-9 relative.
"""
import argparse
import base64
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, n, objective, a0, etamu, first seed, recorded generations)
STEPS = [
    ("n2_rosenbrock", 2, "rosenbrock", 1., 1., 21, [1, 2, 3, 10, 30]),
    ("n5_rosenbrock", 5, "rosenbrock", 0.5, 0.9, 22, [1, 2, 3, 10, 20]),
    ("n12_ellipsoid", 12, "ellipsoid", 1., 1., 23, [1, 2, 3, 12]),
    ("n33_rosenbrock", 33, "rosenbrock", 2., 1., 24, [1, 2, 5]),
]
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
           "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}
RUN_SEEDS = list(range(401, 417))
RUN_N, RUN_TOL, RUN_MFEV = 10, 1e-8, 400000
BUDGET_RUN = (10, 1e-8, 505, 431)       # n, tol, mfev, seed
MIN_GAP = 1e-9
FLOAT_KEYS = ("arx", "fit_val", "xmean", "sigma", "gsigma", "B")

HARNESS = r"""
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "objectives.h"
#include "random.hpp"
#include "multivariate/nes/xnes.h"

using Random = effolkronium::random_static;

struct Probe: public xNES {
    using xNES::xNES;
    void vec(const char *k, const std::vector<double> &v)
    {
        printf("\"%s\":[", k);
        for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
        printf("],");
    }
    // the draws of the next iterate(), on copies of the engine and of the distribution
    void peek()
    {
        auto eng = Random::get_engine();
        auto dist = _Z;
        std::vector<double> z;
        for (int i = 0; i < _np * _n; i++) z.push_back(dist(eng));
        vec("z", z);
    }
    void dump(int gen)
    {
        std::vector<double> arx, arz, fv, B;
        for (auto &p : _points) {
            arx.insert(arx.end(), p._x.begin(), p._x.end());
            arz.insert(arz.end(), p._z.begin(), p._z.end());
            fv.push_back(p._f);
        }
        for (auto &r : _B) B.insert(B.end(), r.begin(), r.end());
        vec("arx", arx); vec("arz", arz); vec("fit_val", fv); vec("xmean", _mu); vec("sigma", { _sigma });
        vec("gsigma", { _Gsigma }); vec("B", B);
        printf("\"np\":%d,\"it\":%d,\"fev\":%d", _np, gen, _fev);
    }
};

struct Ctx { int obj, n; std::vector<double> aux; };

int main(int argc, char **argv)
{
    // steps <obj> <n> <a0> <etamu> <seed> <gens>
    // run   <n> <tol> <mfev> <seed>
    // time  <n> <gens>
    if (!strcmp(argv[1], "time")) {
        const int n = atoi(argv[2]), gens = atoi(argv[3]);
        Ctx c { BBO_OBJ_ROSENBROCK, n, std::vector<double>(n, 0.) };
        Random::seed(1u);
        std::vector<double> lo(n, -5.), up(n, 5.), guess(n, 0.);
        multivariate f = [&c](const double *x) { return bbo_objective_eval(c.obj, c.n, x, c.aux.data()); };
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Probe p(1000000000, 0.);
        p.init(prob, guess.data());
        p.iterate();
        const auto t0 = std::chrono::steady_clock::now();
        for (int g = 0; g < gens; g++) p.iterate();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("{\"n\":%d,\"generations\":%d,\"reference_ms_per_generation\":%.4f}\n", n, gens, ms / gens);
    } else if (!strcmp(argv[1], "steps")) {
        Ctx c { atoi(argv[2]), atoi(argv[3]), {} };
        const int n = c.n, gens = atoi(argv[7]);
        c.aux.resize(n);
        bbo_objective_aux(c.obj, n, c.aux.data());
        Random::seed((unsigned) atoi(argv[6]));
        std::vector<double> lo(n, -5.), up(n, 5.), guess(n, 0.);
        multivariate f = [&c](const double *x) { return bbo_objective_eval(c.obj, c.n, x, c.aux.data()); };
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Probe p(1000000000, 0., atof(argv[4]), atof(argv[5]));
        p.init(prob, guess.data());
        printf("{\"states\":[");
        for (int g = 1; g <= gens; g++) {
            printf("%s{\"gen\":%d,", g > 1 ? "," : "", g);
            p.peek();
            p.iterate();
            p.dump(g);
            printf("}");
        }
        printf("]}\n");
    } else {
        const int n = atoi(argv[2]);
        Ctx c { BBO_OBJ_ROSENBROCK, n, std::vector<double>(n, 0.) };
        Random::seed((unsigned) atoi(argv[5]));
        std::vector<double> lo(n, -5.), up(n, 5.), guess(n, 0.);
        multivariate f = [&c](const double *x) { return bbo_objective_eval(c.obj, c.n, x, c.aux.data()); };
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Probe p(atoi(argv[4]), atof(argv[3]));
        const auto sol = p.optimize(prob, guess.data());
        printf("{\"seed\":%d,\"fev\":%d,\"converged\":%d,\"f\":\"%a\"}\n", atoi(argv[5]), sol._fev,
                sol._converged ? 1 : 0, f(sol._sol.data()));
    }
    return 0;
}
"""


def _floats(hexes):
    return [float.fromhex(v) for v in hexes]


def _pack(values):
    """a list of floats as base64 of their little-endian IEEE doubles"""
    return base64.b64encode(struct.pack("<%dd" % len(values), *values)).decode()


def _min_gap(values):
    """smallest relative gap between neighbours of the sorted values"""
    v = sorted(values)
    gap = float("inf")
    for a, b in zip(v, v[1:]):
        gap = min(gap, (b - a) / max(abs(a), abs(b), 1e-300))
    return gap


def _fit_idx(z, arz, np_, n):
    """the sampling index of every ranked point: its z is one row of the draws"""
    rows = {tuple(z[i * n:(i + 1) * n]): i for i in range(np_)}
    assert len(rows) == np_
    return [rows[tuple(arz[k * n:(k + 1) * n])] for k in range(np_)]


def _build(ref, tmp):
    src = os.path.join(ref, "src")
    with open(os.path.join(tmp, "harness.cpp"), "w") as fh:
        fh.write(HARNESS)
    exe = os.path.join(tmp, "harness")
    subprocess.check_call(
        ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I" + src,
         "-I" + os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(tmp, "harness.cpp"),
         os.path.join(src, "blas.cpp"), os.path.join(src, "multivariate/nes/xnes.cpp"), "-lm"])
    return exe


def time_reference(ref="/root/reference"):
    tmp = tempfile.mkdtemp(prefix="xnes_golden_")
    try:
        exe = _build(ref, tmp)
        for n, gens in ((128, 40), (512, 3)):
            print(subprocess.check_output([exe, "time", str(n), str(gens)]).decode().strip(), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def generate(ref="/root/reference"):
    tmp = tempfile.mkdtemp(prefix="xnes_golden_")
    try:
        exe = _build(ref, tmp)
        steps = []
        for name, n, obj, a0, etamu, seed0, recorded in STEPS:
            for seed in range(seed0, seed0 + 50 * 100, 100):
                out = subprocess.check_output(
                    [exe, "steps", str(OBJ_IDS[obj]), str(n), repr(a0), repr(etamu), str(seed), str(max(recorded))])
                rec = json.loads(out)
                if all(_min_gap(_floats(st["fit_val"])) > MIN_GAP for st in rec["states"] if st["gen"] in recorded):
                    break
                print("%s: seed %d has fitness values closer than %g, trying the next" % (name, seed, MIN_GAP))
            else:
                sys.exit("%s: no tie-free seed" % name)
            np_ = rec["states"][0]["np"]
            for st in rec["states"]:
                z, arz = _floats(st.pop("z")), _floats(st.pop("arz"))
                if st["gen"] in recorded:
                    st["fit_idx"] = _fit_idx(z, arz, np_, n)
                    for k in FLOAT_KEYS:
                        st[k] = _pack(_floats(st[k]))
                else:
                    for k in FLOAT_KEYS + ("it", "fev"):
                        del st[k]
                del st["np"]
                st["z"] = _pack(z)
            rec.update({"name": name, "n": n, "np": np_, "objective": obj, "a0": a0, "etamu": etamu, "seed": seed,
                        "recorded": recorded})
            steps.append(rec)

        def run(n, tol, mfev, seed):
            r = json.loads(subprocess.check_output([exe, "run", str(n), repr(tol), str(mfev), str(seed)]))
            r["f"] = float.fromhex(r["f"]).hex()
            return r

        budget = run(*BUDGET_RUN)
        budget.update({"n": BUDGET_RUN[0], "tol": BUDGET_RUN[1], "mfev": BUDGET_RUN[2]})
        runs = {"objective": "rosenbrock", "n": RUN_N, "tol": RUN_TOL, "mfev": RUN_MFEV, "a0": 1., "etamu": 1.,
                "converging": [run(RUN_N, RUN_TOL, RUN_MFEV, s) for s in RUN_SEEDS], "budget": budget}
        return {"steps": steps, "runs": runs}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "xnes_runs.json"))
    ap.add_argument("--time", action="store_true", help="time the reference instead of writing the fixture")
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
