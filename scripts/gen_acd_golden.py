#!/usr/bin/env python3
"""Records runs of the REAL ACD of the reference into tests/golden/acd_runs.json (needs the reference's
sources and g++; run on the development machine, never where the GPU tests run).

    python scripts/gen_acd_golden.py [--ref /root/reference] [--out tests/golden/acd_runs.json]
    python scripts/gen_acd_golden.py --time      # the reference's us per coordinate step, one core

A small harness (the C++ text below, this project's own) is compiled in a temporary directory against the
reference's acd.cpp with the flags of oracle/Makefile (-O2 -ffp-contract=off).  It seeds
effolkronium::random_static::seed(k) and drives a subclass probe (the members of ACD are protected).

"steps": per shape x_best and sigma after init() and, for each coordinate step of the first SWEEPS sweeps,
both points with their values, f_best, sigma[ix] and `improved` behind the step; behind every updateAE()
`order`, m, p, C, B, invB, diagd and the reference's own residuals ||B B^T - C||_F / ||C||_F (C: its lower
triangle mirrored, what tred2 reads) and ||invB B - I||_max.  A shape's seed moves on until no comparison
the algorithm makes is closer than 1e-6 relative: f1 and f2 against f_best and every adjacent pair of the
sorted archive at each update.  Among the seeds that pass, the one that adds most to the paths still short
of two occurrences is kept; the paths (x1 alone wins, x2 alone wins, both win, neither wins, a clamp that
binds) must each occur at least twice over all shapes.  If no seed passes at the full number of sweeps the
shape is recorded with fewer (at least 2: one real update) and its "note" says so; so it does when the
fixture would otherwise pass MAX_BYTES.  A run is stored in the compact, lossless form of
tests/acd_model.py (pack_run / unpack_run): a point as the coordinates that differ from x_best or, where it
is dense, as what the recorded x_best, sigma and B give plus the coordinates that differ; C as what the
recorded p and the C before give plus the entries that differ; B and invB as one matrix V they both follow
from bit for bit; and checksums of the reference's own points and C that the unpacked numbers must meet.
"bands": n = 10, box +-5, ftol = xtol = 1e-10 on sphere, rosenbrock and schwefel12, 256 seeds each: the sorted
n_evals, the sorted final f_best and the converged share; mfev doubles from 20000 until at least 90 % of the
runs of every objective stop on a tolerance.
"signature": the argument names and defaults of ACD's constructor as bound at py/multivariate_py.cpp:44-48.
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

# (name, n, objective, seed)
SHAPES = [
    ("n1_sphere", 1, "sphere", 11),
    ("n2_rosenbrock", 2, "rosenbrock", 22),
    ("n3_ellipsoid", 3, "ellipsoid", 33),
    ("n5_rosenbrock", 5, "rosenbrock", 44),
    ("n9_schwefel12", 9, "schwefel12", 55),
    ("n17_ellipsoid", 17, "ellipsoid", 66),
    ("n33_schwefel12", 33, "schwefel12", 77),
]
SWEEPS = 4
BOX = 5.
MIN_GAP = 1e-6
SEEDS_TRIED = 128
MAX_BYTES = 466942          # the largest fixture of tests/golden (cma_runs.json)
PATHS = ("x1", "x2", "x1x2", "none", "clamp")
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
           "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}
BANDS = dict(n=10, box=5., ftol=1e-10, xtol=1e-10, mfev=20000, seed0=1000, count=256,
             objectives=["sphere", "rosenbrock", "schwefel12"], share=0.9)
SIGNATURE = [{"name": "mfev", "required": True, "default": None},
             {"name": "ftol", "required": True, "default": None},
             {"name": "xtol", "required": True, "default": None},
             {"name": "ksucc", "required": False, "default": 2.0},
             {"name": "kunsucc", "required": False, "default": 0.5}]

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
#include "multivariate/acd/acd.h"

using Random = effolkronium::random_static;

static void vec(const char *k, const std::vector<double> &v, bool last = false)
{
    printf("\"%s\":[", k);
    for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
    printf("]%s", last ? "" : ",");
}

static std::vector<double> flat(const std::vector<std::vector<double>> &m)
{
    std::vector<double> v;
    for (auto &r : m) v.insert(v.end(), r.begin(), r.end());
    return v;
}

struct Probe: public ACD {
    using ACD::ACD;
    int n() const { return _n; }
    int ix() const { return _ix; }
    int itae() const { return _itae; }
    int fev() const { return _fev; }
    bool improved() const { return _improved; }
    double fbest() const { return _fbest; }
    double sigma(int i) const { return _sigma[i]; }
    void dump_init()
    {
        vec("xbest", _xbest); vec("sigma", _sigma);
        printf("\"cp\":%d", _convergeperiod);
    }
    // ||B B^T - C||_F / ||C||_F over the lower triangle of C mirrored, ||invB B - I||_max
    void residuals(double &r1, double &r2) const
    {
        double num = 0., den = 0.;
        r2 = 0.;
        for (int i = 0; i < _n; i++)
            for (int j = 0; j < _n; j++) {
                double bb = 0., ib = 0.;
                for (int k = 0; k < _n; k++) {
                    bb += _b[i][k] * _b[j][k];
                    ib += _invB[i][k] * _b[k][j];
                }
                const double cij = j <= i ? _c[i][j] : _c[j][i];
                num += (bb - cij) * (bb - cij);
                den += cij * cij;
                r2 = std::max(r2, std::fabs(ib - (i == j ? 1. : 0.)));
            }
        r1 = std::sqrt(num) / std::sqrt(den);
    }
    void dump_update()
    {
        printf("\"order\":[");
        for (size_t i = 0; i < _order.size(); i++) printf("%s%d", i ? "," : "", _order[i]);
        printf("],");
        vec("m", _m);
        if (_itae > 1) {
            double r1, r2;
            residuals(r1, r2);
            vec("p", _p); vec("C", flat(_c)); vec("B", flat(_b)); vec("invB", flat(_invB)); vec("diagd", _diagd);
            printf("\"res_bbt\":\"%a\",\"res_inv\":\"%a\",", r1, r2);
        }
        printf("\"itae\":%d", _itae);
    }
};

struct Ctx { int obj, n; std::vector<double> aux; std::vector<double> log; bool keep; };

int main(int argc, char **argv)
{
    // steps <obj> <n> <box> <seed> <sweeps>
    // bands <obj> <n> <box> <mfev> <ftol> <xtol> <seed0> <count>
    // time  <obj> <n> <iterations>
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
        const double box = atof(argv[4]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed((unsigned) atoi(argv[5]));
        Probe p(1 << 30, 0., 0.);
        p.init(prob, guess.data());
        printf("{\"init\":{");
        p.dump_init();
        printf("},\"steps\":[");
        const int its = atoi(argv[6]) * n;
        c.keep = true;
        for (int g = 0; g < its; g++) {
            const int ix = p.ix(), itae = p.itae();
            c.log.clear();
            p.iterate();
            printf("%s{", g ? "," : "");
            vec("evals", c.log);
            printf("\"fbest\":\"%a\",\"sigma\":\"%a\",\"improved\":%d", p.fbest(), p.sigma(ix), p.improved() ? 1 : 0);
            if (p.itae() != itae) {
                printf(",\"update\":{");
                p.dump_update();
                printf("}");
            }
            printf("}");
        }
        printf("]}\n");
    } else if (!strcmp(argv[1], "bands")) {
        const double box = atof(argv[4]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        const int seed0 = atoi(argv[8]), count = atoi(argv[9]);
        std::vector<double> fb;
        std::vector<int> fev(count), conv(count);
        for (int s = 0; s < count; s++) {
            Random::seed((unsigned) (seed0 + s));
            Probe p(atoi(argv[5]), atof(argv[6]), atof(argv[7]));
            const auto sol = p.optimize(prob, guess.data());
            fb.push_back(p.fbest());
            fev[s] = p.fev();
            conv[s] = sol._converged ? 1 : 0;
        }
        printf("{");
        vec("fbest", fb);
        printf("\"fev\":[");
        for (int s = 0; s < count; s++) printf("%s%d", s ? "," : "", fev[s]);
        printf("],\"converged\":[");
        for (int s = 0; s < count; s++) printf("%s%d", s ? "," : "", conv[s]);
        printf("]}\n");
    } else {
        std::vector<double> lo(n, -5.), up(n, 5.), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed(1u);
        const int its = atoi(argv[4]);
        Probe p(1 << 30, 0., 0.);
        p.init(prob, guess.data());
        for (int g = 0; g < 2 * n; g++) p.iterate();
        const int itae0 = p.itae();
        const auto t0 = std::chrono::steady_clock::now();
        for (int g = 0; g < its; g++) p.iterate();
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        printf("{\"us_per_iteration\":%.6f,\"updates\":%d}\n", us / its, p.itae() - itae0);
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
         os.path.join(src, "multivariate/acd/acd.cpp"), os.path.join(src, "blas.cpp"), "-lm"])
    return exe


def acd_short(h):
    import acd_model
    return acd_model._short(h)


def _hx(v):
    return [float.fromhex(s) for s in v]


def _gap(a, b):
    if a == b:
        return 0.
    if a in (float("inf"), -float("inf")) or b in (float("inf"), -float("inf")):
        return float("inf")
    return abs(a - b) / max(abs(a), abs(b))


def walk(rec, n, box):
    """the smallest relative gap of any comparison the recorded run made, and the paths it met"""
    fbest = float("inf")
    margin = float("inf")
    paths = dict.fromkeys(PATHS, 0)
    fx = [None] * (2 * n)
    for g, st in enumerate(rec["steps"]):
        ix = g % n
        ev = _hx(st["evals"])
        x1, f1, x2, f2 = ev[:n], ev[n], ev[n + 1:2 * n + 1], ev[2 * n + 1]
        margin = min(margin, _gap(f1, fbest))
        w1 = f1 < fbest
        if w1:
            fbest = f1
        margin = min(margin, _gap(f2, fbest))
        w2 = f2 < fbest
        if w2:
            fbest = f2
        assert fbest == float.fromhex(st["fbest"])
        paths["x1x2" if w1 and w2 else "x1" if w1 else "x2" if w2 else "none"] += 1
        if any(abs(v) == box for v in x1 + x2):
            paths["clamp"] += 1
        fx[2 * ix], fx[2 * ix + 1] = f1, f2
        if "update" in st:
            fs = sorted(fx)
            margin = min([margin] + [_gap(a, b) for a, b in zip(fs, fs[1:])])
    return margin, paths


def record(exe, shape, have, sweeps):
    name, n, obj, seed = shape
    best = None
    for attempt in range(SEEDS_TRIED):
        used = seed + 1000 * attempt
        out = subprocess.check_output([exe, "steps", str(OBJ_IDS[obj]), str(n), repr(BOX), str(used), str(sweeps)])
        rec = _norm(json.loads(out))
        margin, paths = walk(rec, n, BOX)
        updates = sum("update" in st for st in rec["steps"])
        if margin < MIN_GAP or updates < min(sweeps, 2):
            continue
        gain = sum(min(paths[k], 2 - min(have.get(k, 0), 2)) for k in PATHS)
        if best is None or (gain, -attempt) > best[0]:
            best = ((gain, -attempt), rec, paths, used, margin, updates)
    if best is None:
        return None
    _, rec, paths, used, margin, updates = best
    rec.update({"name": name, "n": n, "objective": obj, "box": BOX, "seed": used, "sweeps": sweeps,
                "paths": paths, "margin": margin.hex(), "updates": updates})
    # the compact form (tests/acd_model.py): lossless, and checked to be
    import acd_model
    packed = acd_model.pack_run(rec)
    assert acd_model.unpack_run(packed) == rec, name
    return packed


def generate(ref="/root/reference"):
    tmp = tempfile.mkdtemp(prefix="acd_golden_")
    try:
        exe = build(ref, tmp)
        steps, have = [], {}
        for shape in SHAPES:
            rec = None
            for sweeps in range(SWEEPS, 1, -1):
                rec = record(exe, shape, have, sweeps)
                if rec is not None:
                    break
            if rec is None:
                sys.exit("%s: no seed without a close decision, even at 2 sweeps" % shape[0])
            if rec["sweeps"] < SWEEPS:
                rec["note"] = "%d sweeps: no seed of %d has %d without a close decision" % (
                    rec["sweeps"], SEEDS_TRIED, SWEEPS)
            for k in PATHS:
                have[k] = have.get(k, 0) + rec["paths"][k]
            steps.append(rec)
        for k in PATHS:
            if have[k] < 2:
                sys.exit("path %s met %d times only" % (k, have[k]))
        b = dict(BANDS)
        mfev = b["mfev"]
        while True:
            outs = {obj: json.loads(subprocess.check_output(
                [exe, "bands", str(OBJ_IDS[obj]), str(b["n"]), repr(b["box"]), str(mfev), repr(b["ftol"]),
                 repr(b["xtol"]), str(b["seed0"]), str(b["count"])])) for obj in b["objectives"]}
            shares = {obj: sum(o["converged"]) / b["count"] for obj, o in outs.items()}
            print("bands: mfev = %d, converged shares %s" % (mfev, shares))
            if min(shares.values()) >= b["share"]:
                break
            mfev *= 2
            if mfev > 20000 * 1024:
                sys.exit("bands: no budget at which 90 % of the runs converge")
        b["mfev"] = mfev
        for obj, o in outs.items():
            b[obj] = {"n_evals": sorted(o["fev"]), "fbest": [acd_short(v.hex()) for v in sorted(_hx(o["fbest"]))],
                      "converged_share": shares[obj]}
        data = {"steps": steps, "bands": b, "signature": SIGNATURE, "paths": have}
        # the size rule: the largest shape gives up sweeps until the fixture fits
        while len(dumps(data)) > MAX_BYTES:
            big = max(steps, key=lambda r: len(json.dumps(r)))
            if big["sweeps"] <= 2:
                sys.exit("the fixture does not fit %d bytes" % MAX_BYTES)
            idx = steps.index(big)
            shape = [s for s in SHAPES if s[0] == big["name"]][0]
            rec = record(exe, shape, {}, big["sweeps"] - 1)
            if rec is None:
                sys.exit("%s: no seed at %d sweeps" % (big["name"], big["sweeps"] - 1))
            rec["note"] = "%d sweeps: with %d the fixture passes %d bytes" % (rec["sweeps"], SWEEPS, MAX_BYTES)
            steps[idx] = rec
            have = {k: sum(r["paths"][k] for r in steps) for k in PATHS}
            data["paths"] = have
            for k in PATHS:
                if have[k] < 2:
                    sys.exit("path %s met %d times only" % (k, have[k]))
        return data
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def time_reference(ref="/root/reference"):
    """us per coordinate step of the reference on one core: the shape of scripts/bench_acd.py"""
    tmp = tempfile.mkdtemp(prefix="acd_time_")
    try:
        exe = build(ref, tmp)
        for obj in ("rosenbrock", "schwefel12"):
            n, its = 128, 128 * 40
            runs = [json.loads(subprocess.check_output([exe, "time", str(OBJ_IDS[obj]), str(n), str(its)]))
                    for _ in range(5)]
            best = min(runs, key=lambda r: r["us_per_iteration"])
            print("n = %d, %s: %.3f us per coordinate step with %d updates in %d steps (best of 5 runs)"
                  % (n, obj, best["us_per_iteration"], best["updates"], its))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "acd_runs.json"))
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
        print("%s: seed %d, %d sweeps, %d updates, margin %.3g, paths %s%s" % (
            rec["name"], rec["seed"], rec["sweeps"], rec["updates"], float.fromhex(rec["margin"]), rec["paths"],
            " -- " + rec["note"] if "note" in rec else ""))
    print("paths over all shapes: %s" % data["paths"])
    print("bands: mfev = %d" % data["bands"]["mfev"])
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
