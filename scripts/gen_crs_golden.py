#!/usr/bin/env python3
"""Records runs of the REAL CRS of the reference into tests/golden/crs_runs.json (needs the reference's
sources and g++; run on the development machine, never where the GPU tests run).

    python scripts/gen_crs_golden.py [--ref /root/reference] [--out tests/golden/crs_runs.json]
    python scripts/gen_crs_golden.py --time      # the reference's us per iteration and evaluation, one core

A small harness (the C++ text below, this project's own) is compiled in a temporary directory against the
reference's crs.cpp with the flags of oracle/Makefile (-O2 -ffp-contract=off).  It seeds
effolkronium::random_static::seed(k) and drives a subclass probe (the members of CrsSearch are protected).

"steps": per shape the sorted pool after init() and, for each of the first 24 iterations, the raw 32-bit
words it took from the global mt19937 (counted on a copy of the engine), every point handed to the
objective in order with its value (the harness's objective wrapper sees them), and after the iteration the
place of the new point in the sorted pool, fev, _trial and _ftrial (stored compactly: compress()).  Every recorded run
is replayed here through tests/crs_model.py over the recorded words and must match bit for bit; the paths
the model met are counted and stored ("paths").  A shape's seed moves on until no two stored values and no
trial value and the worst are within 1e-6 relative (no tie, no close decision); among the seeds that pass,
the one that adds most to the paths still short of two occurrences is kept.  At n = 1 and n = 2 the rule cannot hold
and is not needed.  At n = 1 the centroid IS the best point, at n = 2 it is the midpoint of the best and
ONE drawn point: a trial that then reflects that same point (one in np) lands on the best point, up to
rounding, is accepted and stores it again, and a pool of 3 or 5 holds values an ulp apart within a few
iterations, whatever the seed.  But the sphere of one coordinate and the Rosenbrock function of two are
ONE term, which the device and the reference round alike, so every value and every decision is the same
bit for bit however close; and at np <= 16 the reference's std::sort is an insertion sort, which puts the
new point behind its equals as the model and the device do.  These two shapes are recorded as they run,
ties and all; a seed is kept only if its recursion stays under depth 64.  A seed on which the reference
itself overflows its stack is skipped.
"bands": the sorted final f(best) of 256 seeds (1000 + s) at a fixed budget with tol = 0 on the sphere and
on Rosenbrock, n = 10, np = 110, and the least, the largest and the mean share of iterations whose
replacement was no better than the worst point ("stale") over the runs.  All 256 runs must end without a crash (the reference
overflows its stack on a collapsed pool); the budget is halved until they do.
"signature": the argument names of CRS's constructor as bound at py/multivariate_py.cpp:339-342.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (name, n, np, objective, box, seed)
SHAPES = [
    ("n1_np3", 1, 3, "sphere", 4., 11),
    ("n2_np5", 2, 5, "rosenbrock", 3., 22),
    ("n3_np7", 3, 7, "ellipsoid", 5., 33),
    ("n5_np20", 5, 20, "rosenbrock", 5., 44),
    ("n9_np20", 9, 20, "sphere", 5., 55),
    ("n17_np40", 17, 40, "ellipsoid", 5., 66),
]
ITERATIONS = 24
MFEV = 1000000
MIN_GAP = 1e-6
SEEDS_TRIED = 24
PATHS = ("B", "mut_acc", "M", "M_stale", "M_inner_mut", "popB_fail", "depth3")
OPTIONAL_PATHS = ("popB_fail",)
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
           "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}
BANDS = dict(n=10, np=110, mfev=4000, tol=0., box=5., seed0=1000, count=256)
SIGNATURE = [{"name": "mfev", "required": True}, {"name": "np", "required": True},
             {"name": "tol", "required": True}]

HARNESS = r"""
#include <algorithm>
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
#include "multivariate/crs/crs.h"

using Random = effolkronium::random_static;

static void vec(const char *k, const std::vector<double> &v, bool last = false)
{
    printf("\"%s\":[", k);
    for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
    printf("]%s", last ? "" : ",");
}

struct Probe: public CrsSearch {
    using CrsSearch::CrsSearch;
    std::vector<double> xs() const
    {
        std::vector<double> x;
        for (auto &p : _points) x.insert(x.end(), p._x.begin(), p._x.end());
        return x;
    }
    std::vector<double> fs() const
    {
        std::vector<double> f;
        for (auto &p : _points) f.push_back(p._f);
        return f;
    }
    int place() const
    {
        for (int i = _np - 1; i >= 0; i--)      // (among identical points the last: the new one)
            if (_points[i]._f == _ftrial && _points[i]._x == _trial) return i;
        return -1;
    }
    void dump_after()
    {
        vec("f", fs()); vec("trial", _trial);
        printf("\"ftrial\":\"%a\",\"slot\":%d,\"fev\":%d", _ftrial, place(), _fev);
    }
    double fbest() const { return _points[0]._f; }
    double fworst() const { return _points[_np - 1]._f; }
    int fev() const { return _fev; }
    // optimize() (:90-102) with the stale replacements counted
    void run(const multivariate_problem &f, const double *guess, int &stale, int &its)
    {
        init(f, guess);
        stale = its = 0;
        while (_fev < _mfev) {
            const double fw = fworst();
            trial();
            if (_ftrial >= fw) stale++;
            update();
            its++;
            if (stop()) break;
        }
    }
    void step() { iterate(); }
};

struct Ctx { int obj, n; std::vector<double> aux; std::vector<double> log; bool keep; };

int main(int argc, char **argv)
{
    // steps <obj> <n> <np> <box> <seed> <iterations> <mfev>
    // bands <obj> <n> <np> <mfev> <tol> <box> <seed0> <count>
    // time  <obj> <n> <np> <iterations>
    Ctx c { atoi(argv[2]), atoi(argv[3]), {}, {}, false };
    const int n = c.n;
    c.aux.resize(n);
    bbo_objective_aux(c.obj, n, c.aux.data());
    multivariate f = [&c](const double *x) {
        const double v = bbo_objective_eval(c.obj, c.n, x, c.aux.data());
        if (c.keep) {
            c.log.insert(c.log.end(), x, x + c.n);
            c.log.push_back(v);
        }
        return v;
    };
    if (!strcmp(argv[1], "steps")) {
        const double box = atof(argv[5]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed((unsigned) atoi(argv[6]));
        Probe p(atoi(argv[8]), atoi(argv[4]), 0.);
        p.init(prob, guess.data());
        printf("{\"init\":{");
        vec("x", p.xs()); vec("f", p.fs());
        printf("\"fev\":%d},\"states\":[", p.fev());
        const int its = atoi(argv[7]);
        c.keep = true;
        for (int g = 1; g <= its; g++) {
            auto before = Random::get_engine();
            c.log.clear();
            p.step();
            const auto after = Random::get_engine();
            printf("%s{\"words\":[", g > 1 ? "," : "");
            for (int i = 0; !(before == after); i++) printf("%s%u", i ? "," : "", (unsigned) before());
            printf("],");
            vec("evals", c.log);
            p.dump_after();
            printf("}");
        }
        printf("]}\n");
    } else if (!strcmp(argv[1], "bands")) {
        const double box = atof(argv[7]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        const int seed0 = atoi(argv[8]), count = atoi(argv[9]);
        std::vector<double> out, fw;
        std::vector<int> stale(count), its(count), fev(count);
        for (int s = 0; s < count; s++) {
            Random::seed((unsigned) (seed0 + s));
            Probe p(atoi(argv[5]), atoi(argv[4]), atof(argv[6]));
            p.run(prob, guess.data(), stale[s], its[s]);
            out.push_back(p.fbest());
            fw.push_back(p.fworst());
            fev[s] = p.fev();
        }
        printf("{");
        vec("fbest", out); vec("fworst", fw);
        const char *names[3] = { "stale", "iterations", "fev" };
        const std::vector<int> *cols[3] = { &stale, &its, &fev };
        for (int k = 0; k < 3; k++) {
            printf("\"%s\":[", names[k]);
            for (int s = 0; s < count; s++) printf("%s%d", s ? "," : "", (*cols[k])[s]);
            printf("]%s", k < 2 ? "," : "");
        }
        printf("}\n");
    } else {
        std::vector<double> lo(n, -5.), up(n, 5.), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed(1u);
        const int its = atoi(argv[5]);
        Probe p(1 << 30, atoi(argv[4]), 0.);
        p.init(prob, guess.data());
        for (int g = 0; g < 100; g++) p.step();
        const int fev0 = p.fev();
        const auto t0 = std::chrono::steady_clock::now();
        for (int g = 0; g < its; g++) p.step();
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        printf("{\"us_per_iteration\":%.6f,\"us_per_evaluation\":%.6f,\"evaluations_per_iteration\":%.4f}\n",
                us / its, us / (p.fev() - fev0), (double) (p.fev() - fev0) / its);
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
         os.path.join(src, "multivariate/crs/crs.cpp"), "-lm"])
    return exe


def _far(a, b):
    return abs(a - b) > MIN_GAP * max(abs(a), abs(b))


def _hx(v):
    return [float.fromhex(s) for s in v]


def checks(rec, n, exact_ok):
    """no tie and no close decision in any recorded state; `exact_ok`: the shape whose bits do not depend
    on either (one-term objectives, see the module's text)"""
    def far(a, b):
        return exact_ok or _far(a, b)
    f = sorted(_hx(rec["init"]["f"]))
    for st in rec["states"]:
        if not all(far(a, b) for a, b in zip(f, f[1:])):
            return False
        ev = _hx(st["evals"])
        if not all(far(ev[k * (n + 1) + n], f[-1]) for k in range(len(ev) // (n + 1))):
            return False
        if st["slot"] < 0:
            return False
        f = _hx(st["f"])
    return all(far(a, b) for a, b in zip(f, f[1:]))


def replay(rec, n, np_, obj, box):
    """the recorded run through tests/crs_model.py over its words: bit for bit, and the paths it met"""
    import chol_model
    import crs_model
    import jaya_model
    m = crs_model.Crs(chol_model.objective(obj, n), n, np_, [-box] * n, [box] * n, MFEV, 0.)
    x0 = _hx(rec["init"]["x"])
    m.start([x0[i * n:(i + 1) * n] for i in range(np_)], _hx(rec["init"]["f"]))
    assert m.order == list(range(np_))
    depth3 = deepest = 0
    for st in rec["states"]:
        w = jaya_model.Words(st["words"])
        assert m.iterate(crs_model.WordsSource(w, n, np_)) and w.exhausted()
        ev = _hx(st["evals"])
        assert [v for x, fx in m.evals for v in x + [fx]] == ev
        assert m.fsorted() == _hx(st["f"]) and m.t == _hx(st["trial"]) and m.ft == float.fromhex(st["ftrial"])
        assert m.slot == st["slot"] and m.fev == st["fev"]
        depth3 += m.maxdepth >= 3
        deepest = max(deepest, m.maxdepth)
    paths = dict(m.paths)
    paths["depth3"] = depth3
    paths["stale"] = m.stale
    paths["maxdepth"] = deepest
    return paths


def compress(rec, n):
    """what the fixture keeps of a recorded run (tests/test_crs_model.py, expand(), puts it back): a point
    handed to the objective a second time in an iteration -- every pop of B does that -- is stored as the
    index of its first entry; _trial and _ftrial as the index of the evaluation they are; the sorted values
    after the last iteration only, since each iteration changes them by _ftrial at "slot" """
    for st in rec["states"]:
        ev, out, seen = st["evals"], [], {}
        for k in range(len(ev) // (n + 1)):
            entry = tuple(ev[k * (n + 1):(k + 1) * (n + 1)])
            if entry in seen:
                out.append(seen[entry])
            else:
                seen[entry] = k
                out.append(list(entry))
        last = tuple(st.pop("trial") + [st.pop("ftrial")])
        st["trial_eval"] = seen[last]           # (KeyError: _trial was not evaluated in this iteration)
        st["evals"] = out
    for st in rec["states"][:-1]:
        del st["f"]


def record(exe, shape, have):
    """one shape: among the seeds without a close decision, the one that adds most to the paths still
    short of two occurrences"""
    name, n, np_, obj, box, seed = shape
    best = None
    for attempt in range(SEEDS_TRIED):
        try:
            out = subprocess.check_output(
                [exe, "steps", str(OBJ_IDS[obj]), str(n), str(np_), repr(box), str(seed + 1000 * attempt),
                 str(ITERATIONS), str(MFEV)])
        except subprocess.CalledProcessError as e:      # (the reference overflowed its stack: a collapsed pool)
            print("%s: seed %d ends the reference with status %s" % (name, seed + 1000 * attempt, e.returncode))
            continue
        rec = _norm(json.loads(out))
        single = (obj == "sphere" and n == 1) or (obj == "rosenbrock" and n == 2)
        if not checks(rec, n, single and np_ <= 16):
            continue
        paths = replay(rec, n, np_, obj, box)
        if single and paths["maxdepth"] >= 64:
            continue
        gain = sum(min(paths[k], 2 - min(have.get(k, 0), 2)) for k in PATHS)
        # (of two seeds that add the same, the first at small n and the shorter record at n >= 9)
        size = len(json.dumps(rec)) if n >= 9 else attempt
        if best is None or (gain, -size) > best[0]:
            best = ((gain, -size), rec, paths, seed + 1000 * attempt)
    if best is None:
        sys.exit("%s: no seed without a close decision" % name)
    _, rec, paths, used = best
    compress(rec, n)
    rec.update({"name": name, "n": n, "np": np_, "objective": obj, "box": box, "mfev": MFEV, "seed": used,
                "paths": paths})
    return rec


def generate(ref="/root/reference"):
    tmp = tempfile.mkdtemp(prefix="crs_golden_")
    try:
        exe = build(ref, tmp)
        steps, have = [], {}
        for shape in SHAPES:
            rec = record(exe, shape, have)
            for k in PATHS:
                have[k] = have.get(k, 0) + rec["paths"][k]
            steps.append(rec)
        for k in PATHS:
            if have[k] < 2:
                if k in OPTIONAL_PATHS:
                    print("path %s: met %d times -- the seeds at these sizes offer no more" % (k, have[k]))
                else:
                    sys.exit("path %s met %d times only" % (k, have[k]))
        bands = dict(BANDS)
        b = BANDS
        mfev = b["mfev"]
        while True:
            try:
                outs = {obj: json.loads(subprocess.check_output(
                    [exe, "bands", str(OBJ_IDS[obj]), str(b["n"]), str(b["np"]), str(mfev), repr(b["tol"]),
                     repr(b["box"]), str(b["seed0"]), str(b["count"])])) for obj in ("sphere", "rosenbrock")}
                break
            except subprocess.CalledProcessError as e:
                print("bands: a reference run ended with status %s at mfev = %d: halving" % (e.returncode, mfev))
                mfev //= 2
                if mfev < 4 * b["np"]:
                    sys.exit("bands: no budget at which all runs end")
        bands["mfev"] = mfev
        for obj, o in outs.items():
            fb = _hx(o["fbest"])
            bands[obj] = [v.hex() for v in sorted(fb)]
            share = [s / i for s, i in zip(o["stale"], o["iterations"])]
            bands[obj + "_stale_share"] = [min(share).hex(), max(share).hex(), (sum(share) / len(share)).hex()]
            bands[obj + "_fworst_min"] = min(_hx(o["fworst"])).hex()
        return {"steps": steps, "bands": bands, "signature": SIGNATURE, "paths": have}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def time_reference(ref="/root/reference"):
    """us per iteration and per evaluation of the reference on one core: the shape of scripts/bench_crs.py"""
    tmp = tempfile.mkdtemp(prefix="crs_time_")
    try:
        exe = build(ref, tmp)
        for n, np_, its in ((128, 1290, 20000),):
            runs = [json.loads(subprocess.check_output(
                [exe, "time", str(OBJ_IDS["rosenbrock"]), str(n), str(np_), str(its)])) for _ in range(5)]
            best = min(runs, key=lambda r: r["us_per_iteration"])
            print("n = %d, np = %d: %.3f us per iteration, %.3f us per evaluation, %.3f evaluations per iteration "
                  "(best of 5 runs of %d)" % (n, np_, best["us_per_iteration"], best["us_per_evaluation"],
                                              best["evaluations_per_iteration"], its))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "crs_runs.json"))
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.ref, "src")):
        sys.exit("the reference sources are not at %s" % a.ref)
    if a.time:
        time_reference(a.ref)
        return
    data = generate(a.ref)
    text = dumps(data)
    with open(a.out, "w") as fh:
        fh.write(text)
    for rec in data["steps"]:
        print("%s: seed %d, paths %s" % (rec["name"], rec["seed"], rec["paths"]))
    print("paths over all shapes: %s" % data["paths"])
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
