#!/usr/bin/env python3
"""Records states of the REAL LmCmaes of the reference into tests/golden/lm_runs.json (needs the
reference's sources and g++).

    python scripts/gen_lm_golden.py [--ref /root/reference] [--out tests/golden/lm_runs.json]

A small harness (the C++ text below, this project's own) is compiled in a temporary directory
against the reference's lm_cmaes.cpp, base_cmaes.cpp and blas.cpp with the flags of oracle/Makefile
(-O2 -ffp-contract=off).  It seeds effolkronium::random_static::seed(k) and drives a probe subclass
generation by generation.  Before every generation the probe copies the engine and replays the
draws the sampler is about to make: per "+" candidate the n values of z (normals, or the +-1 of the
Rademacher coin) and the normal g of selectSubset (0 where the reference draws none).  The fixture
holds numbers and names only.  To keep it small an array of floats is ONE string: base64 of its
little-endian IEEE doubles (tests/test_lm_model.py, `unpack`); a Rademacher row is a string of '+' and
'-'; the scalar outcomes of "runs" are float.hex strings as in the other fixtures.

"steps": five runs (STEPS below); every generation keeps its draws (`z`, `g`), the listed generations the whole
state under the reference's names (arx fit_val fit_idx xmean sigma pc s memlen jarr larr b d pcmat
vmat fp it fev flag; of pcmat and vmat the first memlen rows, the others are still zeros).
"runs": outcomes of complete runs, 16 seeds each of the sphere n = 10, lambda = 12, tol = 1e-8 with
Gaussian and with Rademacher sampling, and one run per stop test ("stops").

Two things are asserted, and the seed of a run is advanced until they hold: no two fitness values
of a generation, nor of the pooled ranking of the sigma rule, are closer than 1e-9 relative; and
every branch of updateSet (filling, removing position k >= 1, dropping slot 0 because every gap is
>= nsteps) occurs in a recorded generation of some run.
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

# (name, n, lambda, objective, rademacher, usenew, bound, box, first seed, start, recorded generations)
STEPS = [
    ("n5_l8_gauss", 5, 8, "rosenbrock", 0, 1, 0, 5., 12, "mid", [1, 2, 3, 5, 6, 7]),
    ("n5_l7_gauss_old", 5, 7, "rosenbrock", 0, 0, 0, 5., 12, "mid", [1, 2, 3, 5, 14]),
    ("n16_l12_rad", 16, 12, "rosenbrock", 1, 1, 0, 5., 14, "mid", [1, 2, 3, 17, 23, 29]),
    ("n16_l12_rad_old", 16, 12, "ellipsoid", 1, 0, 1, 3., 14, "corner", [1, 2, 3, 9, 15]),
    ("n33_l10_rad", 33, 10, "cigar", 1, 1, 0, 5., 15, "mid", [1, 2, 3, 34, 40]),
]
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
           "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}
RUN_SEEDS = list(range(201, 217))
# the stop flags: the CMA engines' codes, 11 = sigma < 1e-16 (include/bbopt_hip.h)
FLAG_NAMES = {1: "MaxIter", 2: "TolHistFun", 3: "EqualFunVals", 11: "SigmaTooSmall"}
# (name, n, lambda, rademacher, mfev, tol, seed)
STOPS = [
    ("maxiter", 10, 12, 1, 120, 1e-8, 301),
    ("tolhistfun", 10, 12, 0, 100000, 1e-8, 302),
    ("sigma", 10, 12, 0, 200000, 0., 303),
    ("equalfunvals", 2, 12, 1, 100000, 1e-8, 304),
]
MIN_GAP = 1e-9
FLOAT_KEYS = ("arx", "fit_val", "xmean", "sigma", "pc", "s", "b", "d", "pcmat", "vmat", "fp")

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "objectives.h"
#include "random.hpp"
#include "multivariate/cma/lm_cmaes.h"

using Random = effolkronium::random_static;

struct Probe: public LmCmaes {
    using LmCmaes::LmCmaes;
    void vec(const char *k, const std::vector<double> &v)
    {
        printf("\"%s\":[", k);
        for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
        printf("],");
    }
    void ints(const char *k, const std::vector<int> &v)
    {
        printf("\"%s\":[", k);
        for (size_t i = 0; i < v.size(); i++) printf("%s%d", i ? "," : "", v[i]);
        printf("],");
    }
    // the draws of the next samplePopulation(), on copies of the engine and of the distribution
    void peek()
    {
        auto eng = Random::get_engine();
        auto dist = _Z;
        const int half = (_lambda + 1) / 2;
        printf("\"draws\":[");
        for (int k = 0; k < half; k++) {
            printf("%s[", k ? "," : "");
            for (int i = 0; i < _n; i++) {
                if (_samplemode == 0) printf("\"%a\",", dist(eng));
                else printf("%d,", std::uniform_real_distribution<double> { 0., 1. }(eng) < 0.5 ? 1 : -1);
            }
            double g = 0.;
            if (_new && _memlen > 1) g = dist(eng);
            printf("\"%a\"]", g);
        }
        printf("],");
    }
    int flag()
    {
        if (_it >= _mit) return 1;
        if (_sigma < _stolmin) return 11;
        if (_it >= _hlen && _fworst - _fbest < _tol) return 2;
        return converged() ? 3 : 0;
    }
    void dump(bool full)
    {
        std::vector<double> arx, fv, pm, vm;
        std::vector<int> fi;
        for (auto &f : _fitness) { fv.push_back(f._value); fi.push_back(f._index); }
        vec("fit_val", fv);
        ints("jarr", _jarr);
        ints("larr", _larr);
        if (full) {
            for (auto &r : _arx) arx.insert(arx.end(), r.begin(), r.end());
            for (auto &r : _pcmat) pm.insert(pm.end(), r.begin(), r.end());
            for (auto &r : _vmat) vm.insert(vm.end(), r.begin(), r.end());
            vec("arx", arx); ints("fit_idx", fi); vec("xmean", _xmean); vec("sigma", { _sigma });
            vec("pc", _pc); vec("s", { _s }); vec("b", _b); vec("d", _d); vec("pcmat", pm);
            vec("vmat", vm); vec("fp", _fp);
            printf("\"fev\":%d,\"flag\":%d,", _fev, flag());
        }
        printf("\"memlen\":%d,\"it\":%d", _memlen, _it);
    }
    int its() const { return _it; }
    int memsize() const { return _memsize; }
    int tt() const { return _t; }
    int nsteps() const { return _nsteps; }
    double fbest() const { return _ybw[0]; }
};

struct Ctx { int obj, n; std::vector<double> aux; };

int main(int argc, char **argv)
{
    // steps <obj> <n> <lambda> <rademacher> <usenew> <bound> <box> <seed> <corner> <mfev> <tol> <gens> <g1,g2,...>
    // run   <n> <lambda> <rademacher> <mfev> <tol> <seed>
    if (!strcmp(argv[1], "steps")) {
        Ctx c { atoi(argv[2]), atoi(argv[3]), {} };
        const int n = c.n, lambda = atoi(argv[4]), rad = atoi(argv[5]), usenew = atoi(argv[6]), bound = atoi(argv[7]);
        const double box = atof(argv[8]);
        const int corner = atoi(argv[10]), gens = atoi(argv[13]);
        std::vector<int> full(gens + 1, 0);
        for (char *t = strtok(argv[14], ","); t; t = strtok(nullptr, ",")) full[atoi(t)] = 1;
        c.aux.resize(n);
        bbo_objective_aux(c.obj, n, c.aux.data());
        Random::seed((unsigned) atoi(argv[9]));
        std::vector<double> lo(n, -box), up(n, box), guess(n);
        for (int i = 0; i < n; i++)
            guess[i] = corner ? box - 0.05 * (1 + i % 3) : Random::get(-3., 3.);
        multivariate f = [&c](const double *x) { return bbo_objective_eval(c.obj, c.n, x, c.aux.data()); };
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Probe p(atoi(argv[11]), atof(argv[12]), lambda, 0, 2., bound != 0, rad != 0, usenew != 0);
        p.init(prob, guess.data());
        printf("{");
        p.vec("guess", guess);
        printf("\"memory\":%d,\"t\":%d,\"nsteps\":%d,\"states\":[", p.memsize(), p.tt(), p.nsteps());
        for (int g = 1; g <= gens; g++) {
            printf("%s{\"gen\":%d,", g > 1 ? "," : "", g);
            p.peek();
            p.iterate();
            p.dump(full[g] != 0);
            printf("}");
        }
        printf("]}\n");
    } else {
        const int n = atoi(argv[2]);
        Ctx c { BBO_OBJ_SPHERE, n, std::vector<double>(n, 0.) };
        Random::seed((unsigned) atoi(argv[7]));
        std::vector<double> lo(n, -10.), up(n, 10.), guess(n);
        for (int i = 0; i < n; i++) guess[i] = Random::get(-3., 3.);
        multivariate f = [&c](const double *x) { return bbo_objective_eval(c.obj, c.n, x, c.aux.data()); };
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Probe p(atoi(argv[5]), atof(argv[6]), atoi(argv[3]), 0, 2., false, atoi(argv[4]) != 0, true);
        const auto sol = p.optimize(prob, guess.data());
        printf("{\"seed\":%d,\"generations\":%d,\"fev\":%d,\"converged\":%d,\"flag\":%d,\"f\":\"%a\"}\n",
                atoi(argv[7]), p.its(), sol._fev, sol._converged ? 1 : 0, sol._converged ? p.flag() : 0, p.fbest());
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


def _pack(hexes):
    """a list of float.hex strings as base64 of their little-endian IEEE doubles"""
    return base64.b64encode(struct.pack("<%dd" % len(hexes), *[float.fromhex(v) for v in hexes])).decode()


def _min_gap(values):
    """smallest relative gap between neighbours of the sorted values"""
    v = sorted(values)
    gap = float("inf")
    for a, b in zip(v, v[1:]):
        gap = min(gap, (b - a) / max(abs(a), abs(b), 1e-300))
    return gap


def _branch(prev_jarr, prev_larr, it, t, m, nsteps):
    """which branch updateSet (lm_cmaes.cpp:274-302) takes in the generation that starts with
    counter `it`: None (not a generation of the memory), "fill", "remove" or "drop0" """
    if it % t:
        return None
    if it // t < m:
        return "fill"
    if m <= 1:
        return "single"
    gaps = [prev_larr[prev_jarr[i + 1]] - prev_larr[prev_jarr[i]] for i in range(m - 1)]
    return "drop0" if min(gaps) >= nsteps else "remove"


def _check(rec, recorded):
    """the two assertions of the module's text for one "steps" run; returns the set of branches the
    recorded generations took, or None when two values lie too close"""
    m, t, nsteps = rec["memory"], rec["t"], rec["nsteps"]
    jarr, larr, fprev = [0] * m, [0] * m, None
    seen = set()
    for st in rec["states"]:
        f = [float.fromhex(v) for v in st["fit_val"]]
        if _min_gap(f) <= MIN_GAP or (fprev is not None and _min_gap(f + fprev) <= MIN_GAP):
            return None
        br = _branch(jarr, larr, st["it"] - 1, t, m, nsteps)
        if br and st["gen"] in recorded:
            seen.add(br)
        jarr, larr, fprev = st["jarr"], st["larr"], f
    return seen


def generate(ref="/root/reference"):
    src = os.path.join(ref, "src")
    tmp = tempfile.mkdtemp(prefix="lm_golden_")
    try:
        with open(os.path.join(tmp, "harness.cpp"), "w") as fh:
            fh.write(HARNESS)
        exe = os.path.join(tmp, "harness")
        subprocess.check_call(
            ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I" + src,
             "-I" + os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(tmp, "harness.cpp"),
             os.path.join(src, "blas.cpp"), os.path.join(src, "multivariate/cma/base_cmaes.cpp"),
             os.path.join(src, "multivariate/cma/lm_cmaes.cpp"), "-lm"])
        steps, branches = [], set()
        for name, n, lam, obj, rad, usenew, bound, box, seed0, start, recorded in STEPS:
            mfev, tol = 1000 * lam, 1e-12
            for seed in range(seed0, seed0 + 50):
                out = subprocess.check_output(
                    [exe, "steps", str(OBJ_IDS[obj]), str(n), str(lam), str(rad), str(usenew), str(bound),
                     repr(box), str(seed), "1" if start == "corner" else "0", str(mfev), repr(tol),
                     str(max(recorded)), ",".join(map(str, recorded))])
                rec = _norm(json.loads(out))
                seen = _check(rec, recorded)
                if seen is not None:
                    break
                print("%s: seed %d has fitness values closer than %g, trying the next" % (name, seed, MIN_GAP))
            else:
                sys.exit("%s: no tie-free seed" % name)
            branches |= seen
            for st in rec["states"]:        # (what only the assertions above needed)
                if st["gen"] not in recorded:
                    for k in ("fit_val", "jarr", "larr", "memlen"):
                        del st[k]
                else:                       # (slots fill in index order: the rows past memlen are zeros)
                    for k in ("pcmat", "vmat"):
                        assert all(float.fromhex(v) == 0. for v in st[k][st["memlen"] * n:])
                        st[k] = st[k][:st["memlen"] * n]
                    for k in FLOAT_KEYS:
                        st[k] = _pack(st[k])
                rows = st.pop("draws")
                st["g"] = _pack([row[-1] for row in rows])
                if rad:
                    st["z"] = ["".join("+" if v == 1 else "-" for v in row[:-1]) for row in rows]
                else:
                    st["z"] = _pack([v for row in rows for v in row[:-1]])
            rec["guess"] = _pack(rec["guess"])
            rec.update({"name": name, "n": n, "lambda": lam, "objective": obj, "rademacher": rad,
                        "usenew": usenew, "bound": bound, "box": box, "seed": seed, "mfev": mfev,
                        "tol": tol, "sigma0": 2.0, "recorded": recorded})
            steps.append(rec)
        missing = {"fill", "remove", "drop0"} - branches
        if missing:
            sys.exit("updateSet branches never recorded: %s" % sorted(missing))

        def run(n, lam, rad, mfev, tol, seed):
            return _norm(json.loads(subprocess.check_output(
                [exe, "run", str(n), str(lam), str(rad), str(mfev), repr(tol), str(seed)])))

        runs = {"objective": "sphere", "n": 10, "lambda": 12, "tol": 1e-8, "sigma0": 2.0, "mfev": 100000,
                "box": 10., "gauss": [run(10, 12, 0, 100000, 1e-8, s) for s in RUN_SEEDS],
                "rademacher": [run(10, 12, 1, 100000, 1e-8, s) for s in RUN_SEEDS], "stops": []}
        for name, n, lam, rad, mfev, tol, seed in STOPS:
            r = run(n, lam, rad, mfev, tol, seed)
            r.update({"name": name, "n": n, "lambda": lam, "rademacher": rad, "mfev": mfev, "tol": tol,
                      "stop": FLAG_NAMES.get(r["flag"], "none")})
            runs["stops"].append(r)
        reached = {r["stop"] for r in runs["stops"]}
        if reached != set(FLAG_NAMES.values()):
            print("stop tests never reached by the reference: %s" % sorted(set(FLAG_NAMES.values()) - reached))
        return {"steps": steps, "runs": runs}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lm_runs.json"))
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.ref, "src")):
        sys.exit("the reference sources are not at %s" % a.ref)
    text = dumps(generate(a.ref))
    with open(a.out, "w") as fh:
        fh.write(text)
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
